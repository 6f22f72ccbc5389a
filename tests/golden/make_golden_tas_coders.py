#!/usr/bin/env python3
"""Generate tests/golden/g13_tas_coders.npz by importing the REAL reference's TasEncoder / TasDecoder.

Run in the build container only (needs /root/reference):

    python tests/golden/make_golden_tas_coders.py

The reference is imported exactly as make_golden.py does (the stand-ins of tests/golden/ref_shim/ for its absent third-party
deps).  The output is data only.  Five geometries (L, N, stride, bias, T), batch 3, K = 2 masks.  To stay far below 1 MB:

  * the input, the masks and the functional's weights r are NOT stored: ``inputs(case)`` below draws them from a seeded
    numpy RandomState (a stream numpy guarantees not to change), and the tests call the same function;
  * results of the fp64 run are stored rounded to fp32 (2^-24 relative: 0.6 % of the tightest gate of 1e-5) except the small
    weight / bias gradients, which stay fp64;
  * a [B, N, T_enc] or [K, B, N, T_enc] tensor of more than ``DENSE`` elements is stored as ``flat[::every]`` with ``every`` odd
    (key ``<name>_every``), so the kept entries walk through all rows and columns; the full tensors are checked against
    torch's fp64 convolutions in tests/test_gpu_tas_coders.py.

Keys per case ``c<i>_``: enc_weight, enc_bias?, dec_weight, dec_bias?, lengths_in, lengths_out, shapes (encoded, decoded),
encoded / decoded / tail (fp64 run), g64_<name> and g32_<name> for name in x, mask, enc_weight, dec_weight, enc_bias, dec_bias:
the gradients of sum(tail * r) from the reference modules in fp64 and in fp32.
"""
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
REPO = HERE.parent.parent

import numpy as np  # noqa: E402

#: (window_length, feature_size, stride, bias, samples)
CASES = [(16, 64, None, False, 2000), (2, 64, None, False, 801), (20, 256, None, True, 1003), (16, 32, 4, False, 1001),
         (5, 7, 3, True, 203)]
BATCH, K, DENSE = 3, 2, 4096


def inputs(index, case, encoded_frames=None, decoded_samples=None):
    """The seeded input ``x [3, T]``, and (once the shapes are known) the masks ``[2, 3, N, T_enc]`` in [0, 1) and ``r [2, 3, T_out]``."""
    L, N, stride, bias, T = case
    rng = np.random.RandomState(1300 + index)
    x = rng.randn(BATCH, T).astype(np.float32)
    if encoded_frames is None:
        return x
    mask = rng.rand(K, BATCH, N, encoded_frames).astype(np.float32)
    r = rng.randn(K, BATCH, decoded_samples).astype(np.float32)
    return x, mask, r


def thin(a):
    """(stored entries, every)."""
    flat = np.asarray(a).reshape(-1)
    every = 1 if flat.size <= DENSE else (-(-flat.size // DENSE)) | 1
    return flat[::every], every


def main():
    sys.path[:0] = [str(HERE / 'ref_shim'), str(REPO), '/root/reference']
    import torch
    from padertorch.contrib.examples.source_separation.tasnet.tas_coders import TasDecoder, TasEncoder  # the reference
    from einops import rearrange

    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)
    out = {}
    for i, case in enumerate(CASES):
        L, N, stride, bias, T = case
        torch.manual_seed(130 + i)
        enc = TasEncoder(window_length=L, feature_size=N, stride=stride, bias=bias)
        dec = TasDecoder(window_length=L, feature_size=N, stride=stride, bias=bias)
        p = f'c{i}_'
        for k, v in list(enc.state_dict().items()) + list(dec.state_dict().items()):
            out[p + k.replace('encoder_1d.', 'enc_').replace('decoder_1d.', 'dec_')] = v.numpy().copy()
        lengths_in = torch.tensor([T, T - 100, T - 150])
        x0 = inputs(i, case)
        with torch.no_grad():
            w0, lengths_out = enc(torch.from_numpy(x0), lengths_in)
            y0 = dec(w0)
        out[p + 'lengths_in'], out[p + 'lengths_out'] = lengths_in.numpy(), lengths_out.numpy()
        out[p + 'shapes'] = np.array([list(w0.shape), [y0.shape[0], y0.shape[1], 0]])
        x0, mask0, r0 = inputs(i, case, w0.shape[2], y0.shape[1])
        for tag, dt in (('64', torch.float64), ('32', torch.float32)):
            e, d = enc.to(dt), dec.to(dt)
            for q in list(e.parameters()) + list(d.parameters()):
                q.grad = None
            x = torch.from_numpy(x0).to(dt).requires_grad_()
            mask = torch.from_numpy(mask0).to(dt).requires_grad_()
            w, _ = e(x)
            tail = d(rearrange(w[None] * mask, 'k b n l -> (k b) n l'))       # tasnet/model.py:119-129
            (tail * torch.from_numpy(r0).to(dt).reshape(tail.shape)).sum().backward()
            if tag == '64':
                with torch.no_grad():
                    out[p + 'decoded'] = d(w).numpy().astype(np.float32)
                out[p + 'tail'] = tail.detach().numpy().astype(np.float32).reshape(r0.shape)
                out[p + 'encoded'], out[p + 'encoded_every'] = thin(w.detach().numpy().astype(np.float32))
            small = dict(enc_weight=e.encoder_1d.weight.grad, dec_weight=d.decoder_1d.weight.grad)
            if bias:
                small.update(enc_bias=e.encoder_1d.bias.grad, dec_bias=d.decoder_1d.bias.grad)
            out[p + f'g{tag}_x'] = x.grad.numpy().astype(np.float32)
            if tag == '64':
                out[p + 'g64_mask'], out[p + 'g64_mask_every'] = thin(mask.grad.numpy().astype(np.float32))
            for k, v in small.items():
                out[p + f'g{tag}_{k}'] = v.numpy().copy()
    out['cases'] = np.array(json.dumps(CASES))
    path = HERE / 'g13_tas_coders.npz'
    np.savez_compressed(path, **out)
    print(path, path.stat().st_size, 'bytes')


if __name__ == '__main__':
    main()
