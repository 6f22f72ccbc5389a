"""The error word of the persistent LSTM kernels.

Contract: ONE int32 word per device that every persistent launch whose bounded spin runs out increments
(``ptmi_lstm_set_error_sink``).  :func:`arm` must have run for a device before its first persistent launch.  The host compares the
word with the count it has already reported: the Trainer stages its value with the gradient norm once per optimizer step
(:func:`error_count` / :func:`errors_since_last_report`), :func:`check_errors` reads it with a host sync.  (Round 1 kept a view of
every call's own error word and folded them with four small torch kernels per check.)
"""
import torch

from .. import _lib

_ERR_SINK = {}      # (device type, index) -> [int32 device tensor [1], count the host has already reported]


def _error_sink(device):
    device = torch.device(device)
    key = _lib.device_key(device)
    ent = _ERR_SINK.get(key)
    if ent is None:
        with torch.cuda.device(key[1]):
            word = torch.zeros(1, dtype=torch.int32, device=device)
            _lib.call('ptmi_lstm_set_error_sink', word.data_ptr())
        ent = _ERR_SINK[key] = [word, 0]
    return ent


def arm(device):
    """Make sure the word a timed-out launch on ``device`` reports to is set (before the first launch)."""
    _error_sink(device)


def error_count(device):
    """0-dim int32 DEVICE tensor: persistent LSTM launches on ``device`` that timed out so far (no kernel, no host sync:
    the caller decides when the value crosses over and hands it to :func:`errors_since_last_report`)."""
    return _error_sink(device)[0][0]


def errors_since_last_report(device, count):
    """``count``: a host copy of :func:`error_count`.  True when it is beyond what has been reported before."""
    ent = _error_sink(device)
    new = int(count) > ent[1]
    ent[1] = max(ent[1], int(count))
    return new


def error_word(device):
    """0-dim int32 DEVICE tensor, non-zero iff a bounded spin of a persistent LSTM kernel on ``device`` ran out and has
    not been reported yet (no host sync)."""
    ent = _error_sink(device)
    return ent[0][0] - ent[1]


def raise_timeout(device):
    raise RuntimeError(
        f'padertorch_amd: a persistent LSTM kernel on {device} timed out waiting for a step counter '
        '(workgroups not co-resident, e.g. the GPU is shared with another long-running kernel). '
        'Set padertorch_amd.ops.lstm.PERSISTENT = False.')


def check_errors():
    """Raise if a bounded spin of a persistent LSTM kernel ran out since the last report (the recurrence results
    are then invalid).  One 4-byte device-to-host copy per device that has run such a kernel."""
    from . import capture as _capture
    if _capture.ACTIVE:         # (a host read: not inside a captured step - GraphedStep stages the word and checks it after the replay)
        return
    for key, ent in list(_ERR_SINK.items()):
        device = torch.device(key[0], key[1])
        if errors_since_last_report(device, int(ent[0])):
            raise_timeout(device)
