"""``beamforming`` of ``padertorch/contrib/jensheit/evaluation.py:14-45`` on the HIP kernels of ``ops.beamforming``: the median of the
masks over the channels, the two PSD matrices (one pass over the observation), the Souden MVDR vector (computed ONCE, reference
channel chosen on the device) and its application to the observation and, when given, to the speech and the noise image.

Same arguments and return triple as the reference, on device tensors instead of numpy arrays: ``...xCxTxF`` complex64 spectra and
float32 masks in, ``...xTxF`` complex64 out.  The reference's ``evaluate_masks`` (PESQ on the host through paderbox) has no
counterpart here.
"""
from ...ops import beamforming as _bf

__all__ = ['beamforming']


def beamforming(observation, speech_mask, noise_mask, speech_image=None, noise_image=None, get_bf_fn=None):
    """
    :param observation: ...xCxTxF
    :param speech_mask: ...xCxTxF
    :param noise_mask: ...xCxTxF
    :param speech_image: ...xCxTxF
    :param noise_image: ...xCxTxF
    :param get_bf_fn: None or ``ops.get_mvdr_vector_souden`` (the reference's default), ``ops.get_gev_vector`` or
        ``ops.get_pca_vector`` (the plain vector, without normalization or phase correction, as the reference would apply it);
        there is no kernel for another vector
    :return: predicted speech signal ...xTxF, and the beamformed speech and noise images (None where no image was given)
    """
    beamformers = {None: 'mvdr_souden', _bf.get_mvdr_vector_souden: 'mvdr_souden', _bf.get_gev_vector: 'gev', _bf.get_pca_vector: 'pca'}
    if get_bf_fn not in beamformers:
        raise NotImplementedError(f'beamforming: only the Souden MVDR, GEV and PCA vectors have a kernel, got get_bf_fn={get_bf_fn!r}')
    if observation.dim() < 3:
        raise ValueError(f'beamforming: ...xCxTxF tensors, got {tuple(observation.shape)}')
    lead, tail = observation.shape[:-3], observation.shape[-3:]

    def rows(x):
        if x.shape != observation.shape:
            raise ValueError(f'beamforming: every tensor of the observation\'s shape {tuple(observation.shape)}, got {tuple(x.shape)}')
        return x.reshape(-1, *tail)
    w, Y, _, _ = _bf.beamforming_vector(rows(observation), rows(speech_mask), rows(noise_mask), beamformer=beamformers[get_bf_fn])

    def apply(x):
        return _bf.apply_beamforming_vector(w, x).reshape(*lead, tail[1], tail[2])
    return (apply(Y), None if speech_image is None else apply(rows(speech_image)),
            None if noise_image is None else apply(rows(noise_image)))
