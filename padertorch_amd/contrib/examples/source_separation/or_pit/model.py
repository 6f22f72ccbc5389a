"""The reference's ``OneAndRestPIT`` (``padertorch/contrib/examples/source_separation/or_pit/model.py:101-422``, "Recursive speech
separation for unknown number of speakers") on the HIP path: a two-output ``TasNet`` is applied recursively, every pass splits one
speaker (``estimate``) from the rest (``residual``), and a flag computed from the separator's additional output says when to stop.

What runs where.  The separator is this package's ``TasNet``.  The flag head (``rearrange`` + ``Linear`` + (weighted) mean + sigmoid in
the reference) is one kernel pair, ``ops.orpit.flag_head``; its weighted modes read the separator's ``mask`` and ``encoded`` directly
(``TasNet.return_mask``), so ``encoded_out = mask * encoded`` is never formed.  The loss of ``review`` (``B x iterations x K`` calls of
``log_mse_loss`` on slices in the reference) is ``ops.orpit.or_pit_iterations``: one statistics pass per iteration for the whole batch,
the choice of the target on the device, one gradient pass.  ``loss`` reads no device value on the host, so ``forward`` + ``loss`` +
backward can be captured in a graph; ``decode`` is the one place that does (its stop condition, ``B == 1``).

Interface: constructor arguments and defaults, ``finalize_dogmatic_config``, the ``state_dict`` keys (``separator.*``, ``flag_nn.weight``,
``flag_nn.bias``: a reference checkpoint loads with ``strict=True``), ``forward`` / ``decode`` / ``review`` and the keys of their dicts
are the reference's.  ``flag_nn`` is a PARAMETER CONTAINER: its own ``forward`` never runs.  ``pre_mean_flag`` is ``[B, E, 1]``.  The
keys ``encoded_out`` / ``encoded_estimate`` / ``encoded_residual`` exist only with the class attribute ``return_encoded`` switched on
(it switches the separator's ``return_encoded_out`` on): nothing here needs them.

Quirks of the reference, handled explicitly:

* ``review`` slices the estimates on the SPEAKER axis (``out[b][:seq_len]``) and the targets on the time axis, so a batch with an
  example shorter than the padded length fails there with a shape error.  Here ``loss`` raises ``ValueError`` unless every entry of
  ``num_samples`` equals ``T`` (lengths given as a GPU tensor are not read, they are taken to be ``T``).
* ``unroll_type='est-silent'`` with ``finetune`` runs one iteration more than there are targets; the reference's ``review`` then
  indexes an empty list (``IndexError``).  The same error is raised here, with a message.
* ``flag_reduction`` ``'min'`` / ``'max'`` call ``torch.min(x, dim=(1, 2))``, a ``TypeError`` in torch: they cannot run.  Here they raise
  ``ValueError`` at construction.
* ``_stop_threshold`` reads ``out['estimated']``, a key that does not exist (``KeyError`` for ``est-silent``); here it reads
  ``out['estimate']``.
* With no estimate at all (``est-silent``, one iteration) ``out`` is zeros ``[B, 0, T]``, here on the input's device, not the CPU.
"""
from typing import Optional

import torch
from torch.nn import functional as F
from torch.nn.utils.rnn import pad_sequence

from ..... import summary
from .....base import Model
from .....ops import orpit
from ..tasnet import TasNet

__all__ = ['OneAndRestPIT']

_UNROLL_TYPES = ('res-single', 'res-silent', 'est-silent')


class OneAndRestPIT(Model):
    #: also return ``encoded_out`` / ``encoded_estimate`` / ``encoded_residual`` per iteration (formed by the separator in plain torch)
    return_encoded: bool = False

    @classmethod
    def finalize_dogmatic_config(cls, config):
        # the separator's additional output feeds the flag; it always has two outputs
        config['separator']['additional_out_size'] = config['flag_units']
        config['separator']['num_speakers'] = 2

    def __init__(
            self,
            separator: TasNet,
            finetune: bool = False,
            unroll_type: str = 'res-single',
            stop_condition: str = 'flag',
            threshold: float = 0.5,
            propagate_grad_between_iterations: bool = False,
            flag_reduction: str = 'mean',
            flag_units: int = 20,
    ) -> None:
        super().__init__()
        if unroll_type not in _UNROLL_TYPES:
            raise ValueError(f'Unknown unroll type: {unroll_type}')
        if flag_reduction in ('min', 'max'):
            raise ValueError(f'flag_reduction={flag_reduction!r} cannot run in the reference (torch.min / torch.max take no tuple of '
                             f'dims) and has no kernel here; use one of {sorted(orpit.FLAG_MODES)}')
        if flag_reduction not in orpit.FLAG_MODES:
            raise ValueError(f'Unknown flag reduction type: {flag_reduction}')
        self.finetune = finetune
        self.unroll_type = unroll_type
        self.threshold = threshold
        self.propagate_grad_between_iterations = propagate_grad_between_iterations
        self.flag_reduction = flag_reduction
        self.flag_units = flag_units

        if stop_condition == 'flag':
            assert flag_units > 0, 'Can\'t use flag stopping criterion if flag is disabled.'
        try:
            self.stop_condition = {
                'threshold': self._stop_threshold,
                'flag': self._stop_flag,
                'none': lambda *x: False,
            }[stop_condition]
        except KeyError:
            raise ValueError(f'Unknown stopping condition: {stop_condition}')

        assert separator.num_speakers == 2, 'The separator has to have two outputs for the OR-PIT!'
        assert flag_units == 0 or separator.additional_out_size == flag_units, (
            f'The separator\'s additional output ({separator.additional_out_size}) has to have flag_units={flag_units} channels')
        self.separator = separator
        # a scalar flag: one output unit
        self.flag_nn = torch.nn.Linear(flag_units, 1) if flag_units > 0 else None

    # ------------------------------------------------------------------------------------------------ forward
    def _forward_step(self, example):
        separator = self.separator
        weighted = self.flag_nn is not None and orpit.FLAG_MODES[self.flag_reduction] is not None
        separator.return_mask = weighted
        if self.return_encoded:
            separator.return_encoded_out = True
        out = separator.forward(example)
        mask = out.pop('mask', None)
        if self.flag_nn is not None:
            encoded = out['encoded'].transpose(1, 2) if weighted and separator.mask else None         # [B, N, E], as the encoder made it
            flag, pre = orpit.flag_head(out['additional_out'], self.flag_nn.weight, self.flag_nn.bias, self.flag_reduction, mask, encoded)
            out['pre_mean_flag'] = pre.unsqueeze(-1)
            out['flag'] = flag
        return out

    def _forward(self, example, max_iterations=4, oracle_num_speakers=None):
        assert oracle_num_speakers is None or oracle_num_speakers <= max_iterations
        y = example['y']
        residual_signal = y if torch.is_tensor(y) and y.dim() == 2 else pad_sequence(list(y), batch_first=True)
        B = residual_signal.shape[0]
        assert B == 1 or oracle_num_speakers is not None, (
            'Counting (when oracle_num_speakers=None) is only supported for a batch-size of 1. Otherwise handling of different numbers '
            'of speakers in the same batch does not work!')

        if oracle_num_speakers is not None:
            last = oracle_num_speakers - {'res-single': 2, 'res-silent': 1, 'est-silent': 0}[self.unroll_type]

            def stop_condition(out, k):
                return k >= last
        else:
            stop_condition = self.stop_condition

        outs = []
        for k in range(max_iterations):
            if not self.propagate_grad_between_iterations:
                residual_signal = residual_signal.detach()
            out = self._forward_step({'y': residual_signal, 'num_samples': example['num_samples']})
            out.update(estimate=out['out'][:, 0], residual=out['out'][:, 1])
            if 'encoded_out' in out:
                out.update(encoded_estimate=out['encoded_out'][:, 0], encoded_residual=out['encoded_out'][:, 1])
            outs.append(out)
            if stop_condition(out, k):
                break
            residual_signal = out['residual']

        estimates = [o['estimate'] for o in outs]
        if self.unroll_type == 'res-single':
            estimates.append(outs[-1]['residual'])
        elif self.unroll_type == 'est-silent':
            estimates = estimates[:-1]
        if len(estimates) == 0:
            estimates = outs[0]['estimate'].new_zeros((B, 0, *outs[0]['estimate'].shape[1:]))
        else:
            estimates = torch.stack(estimates, dim=1)                                                       # [B, K', T]
        return {'out': estimates, 'outs': outs}

    def forward(self, example):
        num_speakers = list(example['num_speakers'])
        assert num_speakers[:-1] == num_speakers[1:], num_speakers
        # 0 forces exactly one iteration
        return self._forward(example, oracle_num_speakers=num_speakers[0] if self.finetune else 0)

    def decode(self, example: dict, max_iterations: int = 4, oracle_num_speakers: Optional[int] = None):
        return self._forward(example, max_iterations, oracle_num_speakers)

    def _stop_threshold(self, out, k):
        if self.unroll_type == 'res-silent':
            return bool(torch.mean(out['residual'] ** 2) < self.threshold)
        if self.unroll_type == 'est-silent':
            return bool(torch.mean(out['estimate'] ** 2) < self.threshold)         # (the reference reads a key 'estimated')
        return False

    def _stop_flag(self, out, k):
        return bool(out['flag'] > self.threshold)

    # ------------------------------------------------------------------------------------------------ loss and review
    def _get_flag_target(self, current_iteration, num_speakers):
        return current_iteration == num_speakers - {'res-single': 2, 'res-silent': 1, 'est-silent': 0}[self.unroll_type]

    def loss(self, inputs: dict, outputs: dict) -> dict:
        """``dict(loss, reconstruction_loss, flag_loss)`` (``flag_loss`` only with a flag) and, detached, ``permutations
        [iterations, B]``: the target every iteration chose.  No device value is read on the host."""
        outs = outputs['outs']
        s = inputs['s']
        if not torch.is_tensor(s):
            s = torch.stack(list(s))
        estimates = [o['out'] for o in outs]
        s = s.to(estimates[0].device)
        B, K, T = s.shape
        lengths = inputs['num_samples']
        if not (torch.is_tensor(lengths) and lengths.is_cuda) and any(int(n) != T for n in lengths):
            raise ValueError(f'OneAndRestPIT.loss: every example has to fill the padded length {T}, got num_samples={list(lengths)} (the '
                             'reference slices the estimates on the speaker axis and fails on such a batch)')
        if len(outs) > K:
            raise IndexError(f'OneAndRestPIT.loss: {len(outs)} iterations for {K} targets: the reference\'s review takes a target off '
                             'an empty list here (unroll_type=\'est-silent\' always runs one iteration more than there are targets)')
        losses, choices = orpit.or_pit_iterations(estimates, s)
        reconstruction_loss = losses.sum() / B
        result = dict(loss=reconstruction_loss, reconstruction_loss=reconstruction_loss, permutations=choices)
        if self.flag_units:
            flag_loss = 0
            for k, out in enumerate(outs):
                flag = out['flag']
                target = torch.ones_like(flag) if self._get_flag_target(k, K) else torch.zeros_like(flag)
                flag_loss = flag_loss + F.binary_cross_entropy(flag, target)
            result.update(loss=reconstruction_loss + flag_loss, flag_loss=flag_loss)
        return result

    def review(self, inputs, outputs):
        losses = self.loss(inputs, outputs)
        outs = outputs['outs']
        s = inputs['s']
        K = len(s[0])
        scalars = {}
        if self.flag_units:
            for k, out in enumerate(outs):
                target_flag = self._get_flag_target(k, K)
                # one value of the batch, for a coarse idea of the flag
                scalars.update({f'flag_value/{target_flag}': out['flag'][0], f'flag_value/{target_flag}/{K}spk': out['flag'][0]})
            scalars.update({'flag_loss': losses['flag_loss'], f'flag_loss/{K}spk': losses['flag_loss']})
        scalars.update({
            'reconstruction_loss': losses['reconstruction_loss'],
            f'loss/{K}spk': losses['loss'],
            f'reconstruction_loss/{K}spk': losses['reconstruction_loss'],
        })
        audios = {
            f'estimate/{K}spk': summary.audio(outs[0]['estimate'][0], sampling_rate=8000),
            f'residual-estimate/{K}spk': summary.audio(outs[0]['residual'][0], sampling_rate=8000),
        }
        return summary.review_dict(scalars=scalars, audios=audios, loss=losses['loss'])
