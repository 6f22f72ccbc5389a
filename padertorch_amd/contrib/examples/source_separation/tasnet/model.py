"""The reference's ``TasNet`` (``padertorch/contrib/examples/source_separation/tasnet/model.py:16-202``) with its whole step on the HIP
path: encoder -> entry norm -> 1x1 conv -> separator -> PReLU -> 1x1 conv -> mask head -> (masked) decoder -> centring, then
``tasnet_loss``.

Layouts: the coders work on ``[B, N, E]`` (channels first), the separator and both projections on ``[B, E, C]`` (channels last).  The
layout changes twice, inside ``ops.tasnet.entry_norm`` and ``ops.tasnet.mask_head``; there is no ``rearrange`` copy and no loop over
the batch, and nothing between the encoder and ``out`` is a torch elementwise, reduction or copy kernel.

Parameters: the reference's names, shapes and order (``state_dict`` and ``named_parameters``), so a reference checkpoint loads with
``strict=True``.  ``encoded_input_norm`` (``torch.nn.LayerNorm``), ``input_proj`` / ``output_proj`` (``torch.nn.Conv1d``) and
``output_prelu`` / ``output_nonlinearity`` are PARAMETER CONTAINERS with the reference's initialisation; their own ``forward`` never runs.

The separator is any module with ``input_size``, ``hidden_size`` and ``forward(x [B, L, N], lengths) -> [B, L, hidden_size]``
(``padertorch_amd.modules.ConvNet``).
"""
from typing import Optional

import torch
from torch.nn.utils.rnn import pad_sequence

from ..... import summary
from .....base import Model
from .....ops import tasnet as glue
from .....ops import tcn
from .....ops.mappings import ACTIVATION_FN_MAP
from .loss import tasnet_loss

__all__ = ['TasNet']

#: the nonlinearity modules the mask head's kernel covers
_HEAD_ACTIVATIONS = {torch.nn.Sigmoid: 'sigmoid', torch.nn.ReLU: 'relu', torch.nn.LeakyReLU: 'leaky_relu', torch.nn.ELU: 'elu',
                     torch.nn.Tanh: 'tanh', torch.nn.Identity: 'identity', torch.nn.PReLU: 'identity'}


class TasNet(Model):
    #: also return ``encoded_out [B, K, E, N]`` (mask * encoded, or the estimate itself with ``mask=False``): the one tensor this path is
    #: built not to form, so it is made - in plain torch, differentiable - only on request (the reference's OR-PIT model reads it)
    return_encoded_out: bool = False
    #: also return ``mask [K, B, N, E]``, the mask head's output as the decoder reads it (the estimate itself with ``mask=False``): no
    #: copy.  The OR-PIT flag head's weighted modes read it together with ``encoded`` instead of ``encoded_out``
    return_mask: bool = False

    def __init__(
            self,
            encoder: torch.nn.Module,
            separator: torch.nn.Module,
            decoder: torch.nn.Module,
            mask: bool = True,
            output_nonlinearity: Optional[str] = 'sigmoid',
            num_speakers: int = 2,
            additional_out_size: int = 0,
            sample_rate: int = 8000,
    ):
        """
        Args:
            encoder: ``TasEncoder`` or ``StftEncoder``
            separator: see the module's docstring
            decoder: ``TasDecoder`` or ``IstftDecoder`` (anything with ``feature_size``, ``forward`` and ``masked``)
            mask: If `True`, use the output of the NN as a mask in tas domain for separation. Otherwise, use the output directly as an
                estimation for the separated signals.
            output_nonlinearity: Nonlinearity applied to the output (right before masking/decoding): 'sigmoid', 'relu', 'leaky_relu',
                'elu', 'tanh', 'identity' or 'prelu'
            num_speakers: The number of speakers/output streams
            additional_out_size: Size of the additional output. Has no effect if set to 0.
            sample_rate: Sample rate of the audio. Only used for correct reporting to TensorBoard.
        """
        super().__init__()

        assert not mask or encoder.feature_size == decoder.feature_size, (
            'Encoder and decoder features sizes must match if masking is '
            'enabled!'
        )
        if output_nonlinearity == 'softmax' or (callable(output_nonlinearity) and not isinstance(output_nonlinearity, str)):
            raise NotImplementedError(
                f'TasNet: output_nonlinearity={output_nonlinearity!r} has no kernel here.  The reference\'s Softmax() is built without a '
                'dim and is applied to a 4-D [K, B, N, L] tensor, where the implicit dim is legacy behaviour of torch (dim=1, the batch '
                'axis) that nobody should rely on; callables cannot be mapped onto the mask head.  Use one of sigmoid, relu, leaky_relu, '
                'elu, tanh, identity, prelu.')
        self.encoder = encoder
        self.separator = separator
        self.decoder = decoder
        self.mask = mask
        self.output_nonlinearity = ACTIVATION_FN_MAP[output_nonlinearity]()
        assert type(self.output_nonlinearity) in _HEAD_ACTIVATIONS, output_nonlinearity
        self.num_speakers = num_speakers
        self.additional_out_size = additional_out_size
        self.sample_rate = sample_rate

        self.encoded_input_norm = torch.nn.LayerNorm(encoder.feature_size)
        self.input_proj = torch.nn.Conv1d(
            encoder.feature_size, separator.input_size, 1)
        self.output_prelu = torch.nn.PReLU()
        self.output_proj = torch.nn.Conv1d(
            separator.hidden_size,
            decoder.feature_size * num_speakers + additional_out_size, 1
        )

    def forward(self, batch: dict) -> dict:
        """``batch['y']``: the mixtures, ``[B, T]`` or a list of ``[T_b]``; ``batch['num_samples']``: their lengths as a list, a CPU tensor
        or a CUDA tensor (then the length arithmetic stays on the device and nothing synchronises: the form to capture in a graph)."""
        y = batch['y']
        sequence = y if torch.is_tensor(y) and y.dim() == 2 else pad_sequence(list(y), batch_first=True)
        sequence_lengths = batch['num_samples']
        if not torch.is_tensor(sequence_lengths):
            sequence_lengths = torch.tensor(sequence_lengths)

        encoded_raw, encoded_sequence_lengths = self.encoder(sequence, sequence_lengths)                    # [B, N, E]
        B, _, E = encoded_raw.shape
        norm = self.encoded_input_norm
        x = glue.entry_norm(encoded_raw, norm.weight, norm.bias, encoded_sequence_lengths, eps=norm.eps)     # [B, E, N]
        x = tcn.pointwise_conv(x, self.input_proj.weight, self.input_proj.bias)
        x = self.separator(x, encoded_sequence_lengths)                                                     # [B, E, hidden]
        x = glue.prelu_rows(x, self.output_prelu.weight)
        z = tcn.pointwise_conv(x, self.output_proj.weight, self.output_proj.bias)                           # [B, E, A + K N]
        activation = _HEAD_ACTIVATIONS[type(self.output_nonlinearity)]
        if isinstance(self.output_nonlinearity, torch.nn.PReLU):
            z = glue.prelu_rows(z, self.output_nonlinearity.weight)
        processed, additional_out = glue.mask_head(z, self.num_speakers, self.decoder.feature_size, self.additional_out_size, activation)
        if processed.shape[-1] != E:
            # the estimation can be longer than the encoded signal (model.py:117); the separators here keep the length
            processed = processed[..., :E]
            additional_out = None if additional_out is None else additional_out[..., :E]

        K = self.num_speakers
        if self.mask:
            assert encoded_raw.shape == processed.shape[1:], (processed.shape, encoded_raw.shape)
            decoded = self.decoder.masked(processed, encoded_raw)                                          # [K, B, T']
        else:
            decoded = self.decoder(processed.reshape(K * B, self.decoder.feature_size, E)).view(K, B, -1)
        out = {
            'out': glue.center(decoded, sequence.shape[-1]),                                               # [B, K, T]
            'encoded': encoded_raw.transpose(1, 2),
            'encoded_sequence_lengths': encoded_sequence_lengths,
        }
        if self.return_encoded_out:
            estimate = encoded_raw.unsqueeze(0) * processed if self.mask else processed
            out['encoded_out'] = estimate.permute(1, 0, 3, 2)                                              # [B, K, E, N]
        if self.return_mask:
            out['mask'] = processed
        if self.additional_out_size > 0:
            out['additional_out'] = additional_out
        return out

    def loss(self, inputs: dict, outputs: dict) -> dict:
        return tasnet_loss(inputs, outputs)

    def review(self, inputs: dict, outputs: dict) -> dict:
        # Report audios
        audios = {
            'observation': summary.audio(signal=inputs['y'][0], sampling_rate=self.sample_rate),
        }
        for i, e in enumerate(outputs['out'][0]):
            audios[f'estimate/{i}'] = summary.audio(signal=e, sampling_rate=self.sample_rate)
        for i, y in enumerate(inputs['s'][0]):
            audios[f'target/{i}'] = summary.audio(signal=y, sampling_rate=self.sample_rate)
        return summary.review_dict(losses=self.loss(inputs, outputs), audios=audios)

    def flatten_parameters(self) -> None:
        if hasattr(self.separator, 'flatten_parameters'):
            self.separator.flatten_parameters()
