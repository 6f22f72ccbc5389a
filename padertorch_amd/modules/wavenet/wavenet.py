"""The WaveNet vocoder of ``padertorch/modules/wavenet/wavenet.py`` on the HIP kernels of ``csrc/wavenet.hip`` (``ops/wavenet.py``): the
reference's constructor, parameter names and shapes (its checkpoints load with ``strict=True``), ``forward`` for training and ``infer``
on this project's own sampling kernel in place of nv-wavenet.

One deviation, on purpose: the reference's ``forward`` applies ``cond_layers`` to the output of ``get_cond_input``, which has applied it
already (wavenet.py:148 after :196) and so raises unless ``n_cond_channels == 2 n_residual_channels n_layers``.  ``infer`` and
``export_weights`` there assume ONE application, and so does this ``forward``.
"""
import torch

from ...base import Module
from ...ops import tcn, wavenet as _wn
from ...ops.mu_law import mu_law_decode

__all__ = ['WaveNet', 'Conv']


class Conv(torch.nn.Module):
    """The parameter holder of the reference's ``Conv``: a ``torch.nn.Conv1d`` under ``.conv`` with Xavier initialisation.  Called on
    ``[B, T, C]`` (channels innermost) it is the 1x1 convolution on the planes GEMM; the dilated convolutions (``kernel_size=2``) run
    inside ``ops.wavenet.residual_stack``."""

    def __init__(self, in_channels, out_channels, kernel_size=1, stride=1, dilation=1, bias=True, w_init_gain='linear', is_causal=False):
        super().__init__()
        self.is_causal = is_causal
        self.kernel_size = kernel_size
        self.dilation = dilation
        self.conv = torch.nn.Conv1d(in_channels, out_channels, kernel_size=kernel_size, stride=stride, dilation=dilation, bias=bias)
        torch.nn.init.xavier_uniform_(self.conv.weight, gain=torch.nn.init.calculate_gain(w_init_gain))

    def forward(self, signal, residual=None):
        if self.kernel_size != 1 or self.conv.stride[0] != 1:
            raise NotImplementedError('Conv: only the 1x1 convolution is a call of its own; the dilated taps run in ops.wavenet.residual_stack')
        return tcn.pointwise_conv(signal, self.conv.weight, self.conv.bias, residual)


class WaveNet(Module):
    def __init__(self, n_cond_channels, upsamp_window, upsamp_stride, n_in_channels=256, n_layers=16, max_dilation=128,
                 n_residual_channels=64, n_skip_channels=256, n_out_channels=256, fading='full'):
        super().__init__()
        _wn.crop_of(fading, upsamp_window, upsamp_stride)
        self.n_layers = n_layers
        self.max_dilation = max_dilation
        self.n_residual_channels = n_residual_channels
        self.n_skip_channels = n_skip_channels
        self.n_in_channels = n_in_channels
        self.n_out_channels = n_out_channels
        self.upsamp_stride = upsamp_stride
        self.upsamp_window = upsamp_window
        self.fading = fading
        self.dilations = _wn.dilations_of(n_layers, max_dilation)

        self.upsample = torch.nn.ConvTranspose1d(n_cond_channels, n_cond_channels, upsamp_window, upsamp_stride)
        self.cond_layers = Conv(n_cond_channels, 2 * n_residual_channels * n_layers, w_init_gain='tanh')
        self.dilate_layers = torch.nn.ModuleList()
        self.res_layers = torch.nn.ModuleList()
        self.skip_layers = torch.nn.ModuleList()
        self.embed = torch.nn.Embedding(n_in_channels, n_residual_channels)
        self.conv_out = Conv(n_skip_channels, n_out_channels, bias=False, w_init_gain='relu')
        self.conv_end = Conv(n_out_channels, n_out_channels, bias=False, w_init_gain='linear')
        for i, dilation in enumerate(self.dilations):
            self.dilate_layers.append(Conv(n_residual_channels, 2 * n_residual_channels, kernel_size=2, dilation=dilation,
                                           w_init_gain='tanh', is_causal=True))
            if i < n_layers - 1:
                self.res_layers.append(Conv(n_residual_channels, n_residual_channels, w_init_gain='linear'))
            self.skip_layers.append(Conv(n_residual_channels, n_skip_channels, w_init_gain='relu'))
        self._packed = None

    # ------------------------------------------------------------------------------------------ training
    def _cond(self, features, out_len=None):
        """``cond_layers(upsample(features))`` as ``[B, T, L 2R]``: channels innermost, layer-major."""
        up = _wn.cond_upsample(features, self.upsample.weight, self.upsample.bias, self.upsamp_stride, self.fading, out_len)
        return self.cond_layers(up)

    def get_cond_input(self, features):
        """``[B, 2 R L, T]`` as the reference returns it (a transposed view of the channels-innermost buffer)."""
        return self._cond(features).transpose(1, 2)

    def forward(self, features, audio):
        """``features [B, C, Tf]``, ``audio [B, T]`` in ``[-1, 1]`` -> ``(output [B, A, T], quantized [B, T] int64)``; ``output[:, :, 0]`` is
        zero and ``output[:, :, t]`` the prediction made from the samples before ``t``."""
        if audio.is_cuda and audio.numel() and not torch.cuda.is_current_stream_capturing():
            assert torch.max(audio) <= 1.0              # the reference's mu_law_encode assertions (host reads)
            assert torch.min(audio) >= -1.0
        x0, quantized = _wn.embed(audio, self.embed.weight)
        B, T = quantized.shape
        front, back = _wn.crop_of(self.fading, self.upsamp_window, self.upsamp_stride)
        have = (features.shape[-1] - 1) * self.upsamp_stride + self.upsamp_window - front - back
        assert self.upsamp_stride > (have - T) >= 0, (tuple(quantized.shape), have)
        cond = self._cond(features, T)
        acts_all = _wn.residual_stack(x0, cond, self.dilations, [m.conv.weight for m in self.dilate_layers],
                                      [m.conv.bias for m in self.dilate_layers], [m.conv.weight for m in self.res_layers],
                                      [m.conv.bias for m in self.res_layers])
        L, R = self.n_layers, self.n_residual_channels
        skip_w = torch.cat([m.conv.weight for m in self.skip_layers], 1)               # [S, L R, 1]: the skip sum is ONE GEMM
        skip_b = torch.stack([m.conv.bias for m in self.skip_layers]).sum(0)
        h = torch.relu(tcn.pointwise_conv(acts_all.view(B, T, L * R), skip_w, skip_b))
        h = torch.relu(self.conv_out(h))
        h = self.conv_end(h)                                                            # [B, T, A]
        shifted = torch.cat((torch.zeros_like(h[:, :1]), h[:, :-1]), 1)
        return shifted.transpose(1, 2), quantized

    # ------------------------------------------------------------------------------------------ inference
    def export_weights(self):
        """The reference's dictionary for an nv-wavenet wrapper (same keys and shapes)."""
        model = {}
        model['embedding_prev'] = torch.zeros(self.n_out_channels, self.n_residual_channels, dtype=torch.float32,
                                              device=self.embed.weight.device)
        model['embedding_curr'] = self.embed.weight.data
        model['conv_out_weight'] = self.conv_out.conv.weight.data
        model['conv_end_weight'] = self.conv_end.conv.weight.data
        model['dilate_weights'] = [m.conv.weight.data for m in self.dilate_layers]
        model['dilate_biases'] = [m.conv.bias.data for m in self.dilate_layers]
        model['max_dilation'] = self.max_dilation
        model['res_weights'] = [m.conv.weight.data for m in self.res_layers]
        model['res_biases'] = [m.conv.bias.data for m in self.res_layers]
        model['skip_weights'] = [m.conv.weight.data for m in self.skip_layers]
        model['skip_biases'] = [m.conv.bias.data for m in self.skip_layers]
        model['use_embed_tanh'] = False
        return model

    def _inference_params(self):
        layers = list(self.dilate_layers) + list(self.res_layers) + list(self.skip_layers) + [self.conv_out, self.conv_end]
        return [p for m in layers for p in m.parameters()]

    def packed_weights(self):
        """The weights in the sampling kernel's form, packed once per parameter version (identity, version and storage of every
        parameter) and cached on the module."""
        params = self._inference_params()
        sig = tuple((id(p), p._version, p.data_ptr()) for p in params)
        if self._packed is None or self._packed[0] != sig:
            w = self.export_weights()
            self._packed = (sig, _wn.pack_inference(w['dilate_weights'], w['dilate_biases'], w['res_weights'], w['res_biases'],
                                                    w['skip_weights'], w['skip_biases'], w['conv_out_weight'], w['conv_end_weight']))
        return self._packed[1]

    def infer(self, x, chunk_length=None, chunk_overlap=0, *, generator=None, selectors=None, return_logits=False, steps_per_launch=None):
        """``x [B, C, Tf]`` features -> audio ``[B, T]`` through ``mu_law_decode``.  ``selectors [B, T]`` in ``[0, 1)`` are the uniforms of
        the inverse-CDF draws (default: drawn with ``generator``).  Chunks are independent restarts, as in the reference, run as further
        sequences of the same launches; of every chunk but the first the leading ``chunk_overlap`` samples are dropped.
        ``return_logits=True``: ``(audio, codes [B, T'], logits [B, T', A])``, the logits the draws were made from."""
        _wn.check_sizes(self.n_residual_channels, self.n_skip_channels, self.n_out_channels)
        if self.n_in_channels < self.n_out_channels:
            raise NotImplementedError(f'WaveNet.infer: {self.n_out_channels} output classes are fed back into an embedding of '
                                      f'{self.n_in_channels} rows')
        from ... import _lib
        _lib.require_gpu(x, selectors)
        with torch.no_grad():
            cond = self._cond(x)
            B, T = cond.shape[:2]
            if selectors is None:
                selectors = torch.rand((B, T), dtype=torch.float32, device=cond.device, generator=generator)
            else:
                if tuple(selectors.shape) != (B, T):
                    raise ValueError(f'WaveNet.infer: selectors {(B, T)}, got {tuple(selectors.shape)}')
                if selectors.dtype != torch.float32:
                    raise NotImplementedError(f'WaveNet.infer: float32 selectors, got {selectors.dtype}')
                if selectors.numel() and not (float(selectors.min()) >= 0.0 and float(selectors.max()) < 1.0):
                    raise ValueError('WaveNet.infer: selectors outside [0, 1)')
            if chunk_length is not None and not 0 <= chunk_overlap < chunk_length:
                raise ValueError(f'WaveNet.infer: chunk_overlap {chunk_overlap} against chunk_length {chunk_length}')
            chunks = _wn.chunks_of(T, chunk_length, chunk_overlap)
            outs = _wn.generate(self.packed_weights(), self.embed.weight.detach(), cond, selectors, self.dilations, self.n_skip_channels,
                                self.n_out_channels, chunks=chunks, steps_per_launch=steps_per_launch, return_logits=return_logits)
            drop = [0] + [chunk_overlap] * (len(chunks) - 1)
            if return_logits:
                codes = torch.cat([c[:, d:] for (c, _), d in zip(outs, drop)], -1)
                logits = torch.cat([lg[:, d:] for (_, lg), d in zip(outs, drop)], 1)
            else:
                codes = torch.cat([c[:, d:] for c, d in zip(outs, drop)], -1)
            audio = mu_law_decode(codes, self.n_out_channels, check=False)
            return (audio, codes, logits) if return_logits else audio
