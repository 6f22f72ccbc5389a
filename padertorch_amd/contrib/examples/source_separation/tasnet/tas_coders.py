"""The coders of the reference's TasNet (``padertorch/contrib/examples/source_separation/tasnet/tas_coders.py``): the learned
filterbank pair ``TasEncoder`` / ``TasDecoder`` (``:9-135``) on the kernels of ``padertorch_amd.ops.tas``, and the STFT pair
(``:138-240``) on the same kernels with a fixed basis (``padertorch_amd.ops.stft_coders``).

``TasEncoder(window_length, feature_size, stride, bias)``: ``[B, T]`` or ``[T]`` -> ``(relu(conv1d) [B, feature_size, frames], lengths)``;
``TasDecoder`` (same arguments): ``[B, feature_size, frames] -> [B, (frames - 1) * stride + window_length]``, and
``TasDecoder.masked(mask [K, B, N, frames], encoded [B, N, frames]) -> [K, B, samples]`` decodes ``mask[k] * encoded`` for every ``k``
without forming the product (the tail of the reference's ``TasNet.forward``, ``tasnet/model.py:119-129``).  Both hold the torch
convolution modules of the reference as PARAMETER CONTAINERS (``encoder_1d`` / ``decoder_1d``: same initialisation, ``state_dict`` keys
and shapes, so reference checkpoints load); the convolutions themselves never run.

``StftEncoder(window_length, feature_size, stride)``: ``[..., T] -> [..., feature_size, frames]`` with the real
parts of the ``feature_size / 2`` bins on top of the imaginary parts; ``IstftDecoder`` is its inverse, and ``IstftDecoder.masked`` has
the contract of ``TasDecoder.masked``.  ``[T]`` / ``[B, T]`` signals and ``[B, N, frames]`` features - what ``TasNet`` passes - run on the
analysis / synthesis kernels of the learned coders with a constant basis (``ops.stft_coders``: designed and measured for TasNet-sized
windows; a dense basis at, say, size 512 / shift 128 is correct but not tuned); inputs with more leading dimensions run on the HIP STFT
(``padertorch_amd.ops.STFT``).  Both paths are differentiable.  The bases are non-persistent buffers: they move with ``.to()``, exist
before a graph capture starts, and are no part of ``state_dict()`` or ``parameters()`` (the reference's coders have neither).  Known
answers held by the reference's doctests (``:140-155``, ``:197-209``) and checked in ``tests/test_gpu_td.py``:
``StftEncoder(feature_size=258)(x[2, 6, 203], [203, 150]) -> [2, 6, 258, 20]`` with ``num_frames == [20, 14]``;
``IstftDecoder(feature_size=258)(X[2, 4, 258, 10]) -> [2, 4, 110]``.
"""
import torch

from .....ops import STFT, stft_coders, tas


class _StftCoder(torch.nn.Module):
    """Shared geometry: an STFT of size ``feature_size - 2`` (an even-sized transform has ``size / 2 + 1`` bins, i.e.
    ``size + 2`` real values per frame), hop ``stride`` (default: half a window), no fading, (re | im) concatenated."""

    def __init__(self, window_length: int = 20, feature_size: int = 256, stride: int = None):
        super().__init__()
        self.window_length, self.feature_size, self.stride = window_length, feature_size, stride
        self.stft = STFT(size=feature_size - 2, shift=window_length // 2 if stride is None else stride,
                         window_length=window_length, fading=False, complex_representation='concat')
        analysis, synthesis = stft_coders.stft_bases(window_length, feature_size, self.stft.shift, self.stft.window)
        self.register_buffer('basis', analysis if self._analysis else synthesis, persistent=False)      # [N, L], fp32


class StftEncoder(_StftCoder):
    _analysis = True

    def forward(self, inputs, sequence_lengths: torch.Tensor = None):
        """Returns the encoded signal, and the frame count of every ``sequence_lengths`` entry when those are given: a CPU int64 tensor
        for a list or a CPU tensor (as the reference); for a CUDA tensor a CUDA tensor, computed on the device without a
        synchronisation (the form to capture in a graph)."""
        if inputs.dim() <= 2:
            encoded = stft_coders.stft_encode(inputs.reshape(-1, inputs.shape[-1]), self.basis, self.stft.shift)    # [B, N, E], contiguous
            encoded = encoded[0] if inputs.dim() == 1 else encoded
        else:
            encoded = self.stft(inputs).transpose(-1, -2)           # frames x bins -> bins x frames
        if sequence_lengths is None:
            return encoded
        return encoded, stft_coders.stft_encoded_lengths(sequence_lengths, self.window_length, self.stft.shift)


class IstftDecoder(_StftCoder):
    _analysis = False

    def forward(self, stft_signal) -> torch.Tensor:
        if stft_signal.dim() == 3:
            return stft_coders.istft_decode(stft_signal, self.basis, self.stft.shift)
        return self.stft.inverse(stft_signal.transpose(-1, -2))

    def masked(self, mask, encoded) -> torch.Tensor:
        """``mask (K, B, N, T_enc)``, ``encoded (B, N, T_enc)`` -> ``(K, B, T)``: ``forward(mask[k] * encoded)`` for every ``k`` in one
        kernel, the product formed on the fly (forward and backward)."""
        return stft_coders.istft_masked_decode(mask, encoded, self.basis, self.stft.shift)


def _default_stride(window_length, stride):
    return window_length // 2 if stride is None else stride


class TasEncoder(torch.nn.Module):
    def __init__(self, window_length: int = 20, feature_size: int = 256, stride: int = None, bias: bool = False):
        super().__init__()
        self.window_length, self.feature_size, self.stride = window_length, feature_size, _default_stride(window_length, stride)
        self.encoder_1d = torch.nn.Conv1d(1, feature_size, window_length, stride=self.stride, padding=0, bias=bias)

    def encoded_lengths(self, sequence_lengths, samples):
        """The reference's frame count of every ``sequence_lengths`` entry of a batch that is ``samples`` long (host arithmetic)."""
        return tas.tas_encoded_lengths(sequence_lengths, samples, self.window_length)

    def forward(self, x, sequence_lengths: torch.Tensor = None):
        """``x (B, T)`` or ``(T,)`` -> ``(w (B, N, T_enc), sequence_lengths in frames or None)``; nothing is masked by the lengths."""
        assert x.dim() in [1, 2], f'The {self.__class__.__name__} ony supports 1D and 2D input, but got {x.shape}.'
        if x.dim() == 1:
            x = x.unsqueeze(0)
        w = tas.tas_encode(x, self.encoder_1d.weight, self.encoder_1d.bias, self.stride, self.window_length)
        return w, self.encoded_lengths(sequence_lengths, x.shape[-1])


class TasDecoder(torch.nn.Module):
    def __init__(self, window_length: int = 20, feature_size: int = 256, stride: int = None, bias=False):
        super().__init__()
        self.window_length, self.feature_size, self.stride = window_length, feature_size, _default_stride(window_length, stride)
        self.decoder_1d = torch.nn.ConvTranspose1d(feature_size, 1, kernel_size=window_length, stride=self.stride, bias=bias)

    def forward(self, w) -> torch.Tensor:
        """``w (B, N, T_enc)`` -> the time signal ``(B, T)``."""
        return tas.tas_decode(w, self.decoder_1d.weight, self.decoder_1d.bias, self.stride)

    def masked(self, mask, encoded) -> torch.Tensor:
        """``mask (K, B, N, T_enc)``, ``encoded (B, N, T_enc)`` -> ``(K, B, T)``: ``forward(mask[k] * encoded)`` for every ``k`` in one
        kernel, the product formed on the fly (forward and backward)."""
        return tas.tas_masked_decode(mask, encoded, self.decoder_1d.weight, self.decoder_1d.bias, self.stride)
