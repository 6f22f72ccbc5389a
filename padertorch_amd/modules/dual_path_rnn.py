"""The dual-path RNN separator (``padertorch/modules/dual_path_rnn.py``: ``DPRNN``, ``DPRNNBlock``, ``_ChunkRNN``, ``segment``,
``overlap_add``; https://arxiv.org/abs/1910.06379) on the kernels of ``padertorch_amd.ops.dprnn`` and the split-fp16 GEMM.

Inside the separator the chunked activation is ``[B, S, K, N]`` (channels last, chunk-major) from segmentation to overlap-add: the
intra-chunk RNN walks its rows with stride 1, the inter-chunk RNN with stride ``K``, and neither transposes (the reference rearranges
four times per block).  The reference's ``[B, N, K, S]`` appears only in the module-level :func:`segment` / :func:`overlap_add`, as a
permuted view.

Sequence lengths: position ``(b, s, k)`` is valid iff ``s < S_b``, the reference's chunk count of example ``b``.  An intra-chunk sequence
``(b, s)`` has ``K`` steps if valid and none otherwise; an inter-chunk sequence ``(b, k)`` has ``S_b`` steps; the norm's output is zero on
invalid positions and the block input is added everywhere - what the reference computes with ``pack`` / ``pack_padded_sequence`` /
``apply_examplewise``.  ``S_b`` is computed on the device; the reference's ``may_deactivate_seq`` shortcut (a host decision with the
same result) is never taken.  Unlike ``pack_padded_sequence`` the lengths need not be sorted.

The modules hold the reference's parameters under the reference's names (``state_dict`` keys, shapes and order), so a reference
checkpoint loads with ``strict=True``; ``rnn`` (``torch.nn.LSTM``), ``fc`` and ``norm`` are parameter containers whose own ``forward``
never runs.
"""
import math
import warnings
from typing import Optional, Tuple

import torch
from torch.nn.utils.rnn import PackedSequence, pad_packed_sequence

from ..base import Module
from ..ops import dprnn as _ops

__all__ = ['DPRNN', 'DPRNNBlock', 'segment', 'overlap_add']


def segment(signal: torch.Tensor, hop_size: int, window_size: int, sequence_lengths: Optional[torch.Tensor] = None
            ) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """``signal ([B,] L, N)`` -> ``([B,] N, K, S)``, zero-padded by ``K - P`` frames at both ends and cut into windows of ``K`` frames
    every ``P`` (``dual_path_rnn.py:24-150``), and the chunk counts ``(len + (K - P) - 1) // P + 1`` of ``sequence_lengths`` (None if not
    given).  The result is a permuted view of the ``[B, S, K, N]`` buffer the kernel writes."""
    batched = signal.dim() == 3
    seg = _ops.segment_rows(signal if batched else signal.unsqueeze(0), window_size, hop_size).permute(0, 3, 2, 1)
    if sequence_lengths is not None:
        sequence_lengths = _ops.chunk_counts(sequence_lengths, window_size, hop_size)
    return (seg if batched else seg[0]), sequence_lengths


def overlap_add(signal: torch.Tensor, hop_size: int, unpad: bool = True) -> torch.Tensor:
    """``signal (B, N, K, S)`` -> ``(B, L, N)``: the windows added at their positions (``dual_path_rnn.py:153-211``); ``unpad`` removes the
    ``K - P`` frames at both ends that :func:`segment` added.  ``unpad=False`` is not differentiable here and raises on an input that
    requires a gradient."""
    if signal.dim() != 4:
        raise ValueError(f'overlap_add: signal (B, N, K, S), got {tuple(signal.shape)}')
    B, N, K, S = signal.shape
    assert K > hop_size
    seg = signal.permute(0, 3, 2, 1)
    if unpad:
        return _ops.overlap_add_rows(seg, hop_size)
    _ops._check('overlap_add', signal)
    if signal.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError('overlap_add: unpad=False has no backward kernel here; use unpad=True or detach the input')
    return torch.ops.ptmi.dprnn_overlap_add(seg, hop_size, S * hop_size + K - hop_size, 0)


_RNN_TYPES = ('lstm', 'blstm', 'cnn', 'gru', 'bgru')


class _ChunkRNN(Module):
    """An RNN, a fully connected layer and a normalisation layer plus the input (``dual_path_rnn.py:284-507``).  ``lstm_reshape_to``
    names the path as in the reference: ``'(b s) k n'`` runs along the chunk (intra), ``'(b k) s n'`` across the chunks (inter).
    ``forward(rows [B S K, N], tables)`` with the tables of :meth:`DPRNN.forward`."""

    def __init__(self, feat_size: int, rnn_size: int, lstm_reshape_to: str, rnn_type='blstm'):
        super().__init__()
        if rnn_type not in _RNN_TYPES:
            raise ValueError(f'Unknown rnn_type for chunk RNN: {rnn_type}')
        if rnn_type in ('gru', 'bgru', 'cnn'):
            raise NotImplementedError(f"_ChunkRNN: rnn_type={rnn_type!r} has no HIP kernel here: the chunk recurrence kernel is an LSTM "
                                      f"cell; use 'lstm' or 'blstm'")
        if lstm_reshape_to.replace(' ', '') not in ('(bs)kn', '(bk)sn'):
            raise NotImplementedError(f"_ChunkRNN: lstm_reshape_to '(b s) k n' (intra-chunk) or '(b k) s n' (inter-chunk), "
                                      f"got {lstm_reshape_to!r}")
        if rnn_size > _ops.MAX_HIDDEN:
            raise NotImplementedError(f'_ChunkRNN: rnn_size {rnn_size} > {_ops.MAX_HIDDEN}: the chunk recurrence kernels take at most '
                                      f'{_ops.MAX_HIDDEN} units (W_hh stays on chip up to {_ops.RESIDENT_HIDDEN} and is streamed above)')
        self.rnn = torch.nn.LSTM(input_size=feat_size, hidden_size=rnn_size, bidirectional=rnn_type == 'blstm', batch_first=True)
        self.fc = torch.nn.Linear(in_features=2 * rnn_size if rnn_type == 'blstm' else rnn_size, out_features=feat_size)
        self.norm = torch.nn.LayerNorm((feat_size,))
        self.lstm_reshape_to = lstm_reshape_to
        self.feat_size = feat_size
        self.intra = lstm_reshape_to.replace(' ', '') == '(bs)kn'

    def forward(self, rows: torch.Tensor, tables) -> torch.Tensor:
        chunks, intra, inter, S, K = tables
        table, cap = (intra, K) if self.intra else (inter, S)
        return _ops.chunk_rnn(rows, table, cap, chunks, S, K, self.rnn, self.fc, self.norm)

    def flatten_parameters(self) -> None:
        """Nothing to do: the parameters are read in place by the kernels."""


class DPRNNBlock(Module):
    """One DPRNN block: an intra-chunk and an inter-chunk RNN (``dual_path_rnn.py:510-547``)."""

    def __init__(self, feat_size: int, rnn_size: int, inter_chunk_type: str = 'blstm', intra_chunk_type: str = 'blstm'):
        super().__init__()
        self.intra_chunk_rnn = _ChunkRNN(feat_size=feat_size, rnn_size=rnn_size, lstm_reshape_to='(b s) k n', rnn_type=intra_chunk_type)
        self.inter_chunk_rnn = _ChunkRNN(feat_size=feat_size, rnn_size=rnn_size, lstm_reshape_to='(b k) s n', rnn_type=inter_chunk_type)

    def forward(self, rows: torch.Tensor, tables) -> torch.Tensor:
        return self.inter_chunk_rnn(self.intra_chunk_rnn(rows, tables), tables)

    def flatten_parameters(self) -> None:
        self.intra_chunk_rnn.flatten_parameters()
        self.inter_chunk_rnn.flatten_parameters()


class DPRNN(Module):
    """The Dual-Path RNN (``dual_path_rnn.py:550-675``), not the source separator around it.

    ``forward(sequence (B, L, N), sequence_lengths=None) -> (B, S P - (K - P), N)`` - at least ``L`` frames, as in the reference.
    ``sequence_lengths``: None, a list, a CPU tensor or a CUDA tensor (then nothing synchronises: the form to capture in a graph)."""

    def __init__(self, input_size: int, rnn_size: int, window_length: int, hop_size: int, num_blocks: int,
                 inter_chunk_type: str = 'blstm', intra_chunk_type='blstm'):
        super().__init__()
        self.window_size = window_length
        self.hop_size = hop_size
        self.input_size = self.hidden_size = input_size
        self.dprnn_blocks = torch.nn.Sequential(*[
            DPRNNBlock(feat_size=input_size, rnn_size=rnn_size, inter_chunk_type=inter_chunk_type, intra_chunk_type=intra_chunk_type)
            for _ in range(num_blocks)])

    def calculate_window_and_hop_size(self, sequence: torch.Tensor, sequence_lengths: Optional[torch.Tensor] = None) -> Tuple[int, int]:
        """The segmentation parameters; ``'auto'``: the heuristic K ~ sqrt(2 L) of the paper, Sec. 2.2."""
        if self.window_size == 'auto' or self.hop_size == 'auto':
            assert self.window_size == self.hop_size == 'auto', 'Set both window_size and hop_size or none of them!'
            assert sequence_lengths is None or len(sequence_lengths) == 1, (
                'Variable length window and hop size (window_size = hop_size = "auto") are not supported (impossible) with non-unique '
                'sequence lengths in one batch! Either supply examples without sequence length or reduce the batch size to 1.')
            window_size = int(math.sqrt(2 * sequence.shape[-2]))
            hop_size = window_size // 2
        else:
            window_size = self.window_size
            hop_size = self.hop_size
        return window_size, hop_size

    def forward(self, sequence: torch.Tensor, sequence_lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
        if isinstance(sequence, PackedSequence):
            warnings.warn('DPRNN does not support packed sequences. Unpacking it again!')
            sequence, sequence_lengths = pad_packed_sequence(sequence, batch_first=True)
        if sequence.dim() != 3 or sequence.shape[2] != self.input_size:
            raise ValueError(f'DPRNN: sequence (B, L, {self.input_size}), got {tuple(sequence.shape)}')
        window_size, hop_size = self.calculate_window_and_hop_size(sequence, sequence_lengths)
        segmented = _ops.segment_rows(sequence, window_size, hop_size)                    # [B, S, K, N]
        B, S, K, N = segmented.shape
        chunks, intra, inter = _ops.tables(segmented, sequence_lengths, B, S, K, hop_size)
        tables = (None if sequence_lengths is None else chunks, intra, inter, S, K)
        h = segmented.view(B * S * K, N)
        for block in self.dprnn_blocks:
            h = block(h, tables)
        return _ops.overlap_add_rows(h.view(B, S, K, N), hop_size)

    def flatten_parameters(self) -> None:
        for block in self.dprnn_blocks:
            block.flatten_parameters()
