#!/usr/bin/env python3
"""Time the TasNet model in the reference's ``convnet`` configuration (``tasnet/train.py:55-68,149-159``: window 16, stride 8, 256
features, ``ConvNet(256, 8, 4, 512, 3, 'gLN')``, K = 2) at B = 4, T = 32 000: forward + loss + backward of the whole model, and of the
glue region alone (entry norm, output PReLU, mask head, centring, each with its backward: csrc/tasnet.hip), on the HIP path and on the
same parameters composed from torch's own operators (F.conv1d, F.layer_norm per example into a zeros buffer, F.prelu, chunk / stack,
torch.sigmoid, F.conv_transpose1d, mean) - our own restatement of ``tasnet/model.py:69-152`` - on the same GPU in the same process.  The
loss of both chains is ``tasnet_loss`` (it is not what is compared).

    python scripts/bench_tasnet.py [--iters 10] [--warmup 3] [--rounds 5] [--out profiles/tasnet.txt]

Method (scripts/bench_convnet.py): every chain is warmed up, then timed in ``rounds`` windows of ``iters`` iterations between two events,
the chains alternating window by window; reported are the median window (us per iteration) and min .. max.  Needs a GPU.
"""
import argparse
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from bench_convnet import library_block, measure  # noqa: E402

B, T, K, L, N = 4, 32000, 2, 16, 256
LENGTHS = [32000, 28000, 24000, 16000]


def library_entry_norm(w, norm, lengths):                    # w [B, N, E] -> [B, E, N]
    x = w.transpose(1, 2)
    out = torch.zeros_like(x)
    for b, n in enumerate(lengths):                          # apply_examplewise (modules/dual_path_rnn.py:258-281)
        out[b, :n] = F.layer_norm(x[b, :n], (x.shape[2],), norm.weight, norm.bias, norm.eps)
    return out


def library_head(z):                                         # z [B, E, K N] -> [K, B, N, E]
    return torch.sigmoid(torch.stack(torch.chunk(z.transpose(1, 2), K, dim=1)))


def library_center(d, samples):                              # d [K, B, T'] -> [B, K, T]
    d = d[..., :samples]
    return (d - torch.mean(d, dim=-1, keepdim=True)).transpose(0, 1)


def library_forward(net, y, enc_lengths):
    w = F.relu(F.conv1d(y[:, None], net.encoder.encoder_1d.weight, None, stride=net.encoder.stride))
    x = library_entry_norm(w, net.encoded_input_norm, enc_lengths)
    x = F.conv1d(x.transpose(1, 2), net.input_proj.weight, net.input_proj.bias)
    for rep in net.separator.conv_blocks:
        for block in rep:
            x = library_block(block, x)
    z = F.conv1d(F.prelu(x, net.output_prelu.weight), net.output_proj.weight, net.output_proj.bias)
    m = torch.sigmoid(torch.stack(torch.chunk(z, K, dim=1)))
    est = (w.unsqueeze(0) * m).reshape(K * y.shape[0], N, -1)
    d = F.conv_transpose1d(est, net.decoder.decoder_1d.weight, None, stride=net.decoder.stride)[:, 0].view(K, y.shape[0], -1)
    return library_center(d, y.shape[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_tasnet.py needs an MI355X'
    from padertorch_amd.contrib.examples.source_separation.tasnet import TasDecoder, TasEncoder, TasNet, tasnet_loss
    from padertorch_amd.modules import ConvNet
    from padertorch_amd.ops import tasnet as glue
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    net = TasNet(TasEncoder(L, N), ConvNet(N, 8, 4, 512, 3, 'gLN'), TasDecoder(L, N), num_speakers=K).to(dev)
    params = list(net.parameters())
    y, s = torch.randn(B, T, device=dev), torch.randn(B, K, T, device=dev)
    lengths = torch.tensor(LENGTHS, device=dev)
    enc_lengths = [int(n) for n in net.encoder.encoded_lengths(torch.tensor(LENGTHS), T)]
    batch = dict(y=y, s=s, num_samples=lengths)

    def hip_step():
        loss = tasnet_loss(batch, net(batch))['si-sdr']
        return [loss.detach()] + list(torch.autograd.grad(loss, params))

    def library_step():
        loss = tasnet_loss(batch, dict(out=library_forward(net, y, enc_lengths)))['si-sdr']
        return [loss.detach()] + list(torch.autograd.grad(loss, params))
    a, b = hip_step(), library_step()
    worst = max(float((p - q).abs().max() / q.abs().max().clamp(min=1e-30)) for p, q in zip(a, b))
    print(f'loss and parameter gradients of the two chains differ by at most {worst:.1e} of their maximum', flush=True)
    lines = [f'# loss and parameter gradients of the two chains differ by at most {worst:.1e} of their maximum']
    assert worst <= 5e-2, worst                              # the two chains compute the same thing (both fp32)
    lines.append(measure(f'TasNet convnet configuration (L {L}, {N} features, ConvNet 8x4 / 512 gLN, K {K}) B={B} T={T}, forward + '
                         'loss + backward', dict(hip=hip_step, library=library_step), args))

    # the glue region alone: its four operators on tensors of the model's shapes, each forward + backward
    E = T // (L // 2) - 1
    norm, slope = net.encoded_input_norm, net.output_prelu.weight
    w = torch.randn(B, N, E, device=dev, requires_grad=True)
    x = torch.randn(B, E, N, device=dev, requires_grad=True)
    z = torch.randn(B, E, K * N, device=dev, requires_grad=True)
    d = torch.randn(K, B, T, device=dev, requires_grad=True)
    r = [torch.randn(B, E, N, device=dev), torch.randn(B, E, N, device=dev), torch.randn(K, B, N, E, device=dev),
         torch.randn(B, K, T, device=dev)]
    len_dev = torch.tensor(enc_lengths, device=dev)
    leaves = [w, x, z, d, norm.weight, norm.bias, slope]

    def hip_glue():
        outs = [glue.entry_norm(w, norm.weight, norm.bias, len_dev, eps=norm.eps), glue.prelu_rows(x, slope),
                glue.mask_head(z, K, N)[0], glue.center(d, T)]
        return torch.autograd.grad(sum((o * q).sum() for o, q in zip(outs, r)), leaves)

    def library_glue():
        outs = [library_entry_norm(w, norm, enc_lengths), F.prelu(x.transpose(1, 2), slope).transpose(1, 2), library_head(z),
                library_center(d, T)]
        return torch.autograd.grad(sum((o * q).sum() for o, q in zip(outs, r)), leaves)
    worst = max(float((p - q).abs().max() / q.abs().max().clamp(min=1e-30)) for p, q in zip(hip_glue(), library_glue()))
    assert worst <= 1e-3, worst
    lines.append(measure(f'glue region (entry norm, PReLU, mask head, centring; + the functional\'s products) {N} features B={B} E={E} '
                         f'T={T}, forward + backward', dict(hip=hip_glue, library=library_glue), args))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
