#!/usr/bin/env python3
"""Generate the training-mode BatchNorm fixtures by running the REFERENCE's own FastGRNNBatchNorm module (its cell
unrolled by BaseRNN, every BatchNorm1d in training mode) in fp64.

Run in the build container only (needs /root/reference, read-only):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/batchnorm/make_bn_train_golden.py

Writes DATA only, next to this script: train_<case>.npz (fp64 results) with

* the inputs: W, U, x, G (the upstream gradient: the loss is sum(hs * G)) as int8 multiples of 2^-e (exact in fp64,
  a quarter of the bytes), h0, bias_gate, bias_update, zeta, nu and, per BatchNorm layer, weight, bias,
  running_mean, running_var (fp64), num_batches_tracked, eps and momentum (NaN: momentum=None);
* the outputs: hs, the gradient of every parameter (d<name>), d_x, d_h0, and every running statistic and
  num_batches_tracked after the forward (post_<bn>_<buffer>).
"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
sys.path.insert(0, "/root/reference")
import rnn  # noqa: E402  (the reference)

HERE = os.path.dirname(os.path.abspath(__file__))
BNS = ("bn_w", "bn_u", "bn_gate", "bn_update")

# name: (F, H, T, B, gate, momentum, eps of bn_u, seed)
CASES = {
    "h128_in32": (32, 128, 12, 16, "sigmoid", 0.1, 1e-5, 21),
    "h256_in64": (64, 256, 12, 5, "tanh", None, 1e-3, 22),
}


def q8(g, shape, e):
    """int8 values times 2^-e: exact in fp64 and fp32."""
    return torch.randint(-100, 101, shape, generator=g, dtype=torch.int64).to(torch.int8), e


def make(name, F, H, T, B, gate, momentum, eps_u, seed):
    torch.set_default_dtype(torch.float64)
    g = torch.Generator().manual_seed(seed)
    m = rnn.FastGRNNBatchNorm(F, H, gate_nonlinearity=gate, update_nonlinearity="tanh")
    cell = m.cell
    qW, eW = q8(g, (F, H), 9)
    qU, eU = q8(g, (H, H), 10)
    qx, ex = q8(g, (T, B, F), 6)
    qG, eG = q8(g, (T, B, H), 6)
    deq = lambda q, e: q.double() * 2.0 ** -e  # noqa: E731
    with torch.no_grad():
        cell.W.copy_(deq(qW, eW))
        cell.U.copy_(deq(qU, eU))
        cell.bias_gate.copy_(0.5 * torch.randn(1, H, generator=g))
        cell.bias_update.copy_(0.5 * torch.randn(1, H, generator=g))
        cell.zeta.fill_(0.8)
        cell.nu.fill_(-2.0)
        for bn in (getattr(cell, n) for n in BNS):
            bn.momentum = momentum
            bn.weight.copy_(1.0 + 0.5 * torch.randn(H, generator=g))
            bn.bias.copy_(0.3 * torch.randn(H, generator=g))
            bn.running_mean.copy_(0.5 * torch.randn(H, generator=g))
            bn.running_var.copy_(0.5 + torch.rand(H, generator=g))
            bn.num_batches_tracked.fill_(7)
        cell.bn_u.eps = eps_u
    pre = {}
    for n in BNS:
        bn = getattr(cell, n)
        for k in ("weight", "bias", "running_mean", "running_var"):
            pre["%s_%s" % (n, k)] = getattr(bn, k).detach().numpy().copy()
        pre["%s_num_batches_tracked" % n] = np.int64(bn.num_batches_tracked.item())
        pre["%s_eps" % n] = np.float64(bn.eps)
        pre["%s_momentum" % n] = np.float64(np.nan if bn.momentum is None else bn.momentum)
    m.train()
    x = deq(qx, ex).requires_grad_(True)
    Gt = deq(qG, eG)
    h0 = (0.5 * torch.randn(B, H, generator=g)).requires_grad_(True)
    hs = m(x, h0.unsqueeze(0).clone(), training=True)
    (hs * Gt).sum().backward()
    out = {"hs": hs.detach().numpy(), "d_x": x.grad.numpy(), "d_h0": h0.grad.numpy()}
    for k in ("W", "U", "bias_gate", "bias_update", "zeta", "nu"):
        out["d" + k] = getattr(cell, k).grad.numpy()
    for n in BNS:
        bn = getattr(cell, n)
        out["d%s_weight" % n] = bn.weight.grad.numpy()
        out["d%s_bias" % n] = bn.bias.grad.numpy()
        out["post_%s_running_mean" % n] = bn.running_mean.numpy()
        out["post_%s_running_var" % n] = bn.running_var.numpy()
        out["post_%s_num_batches_tracked" % n] = np.int64(bn.num_batches_tracked.item())
    np.savez_compressed(os.path.join(HERE, "train_%s.npz" % name),
                        qW=qW.numpy(), eW=np.int64(eW), qU=qU.numpy(), eU=np.int64(eU), qx=qx.numpy(),
                        ex=np.int64(ex), qG=qG.numpy(), eG=np.int64(eG), h0=h0.detach().numpy(),
                        bias_gate=cell.bias_gate.detach().numpy(), bias_update=cell.bias_update.detach().numpy(),
                        zeta=cell.zeta.detach().numpy(), nu=cell.nu.detach().numpy(),
                        meta_gate=np.array(gate), **pre, **out)
    print("%s: max|hs| %.3g, max|dU| %.3g" % (name, float(hs.detach().abs().max()), float(np.abs(out["dU"]).max())))


if __name__ == "__main__":
    for name, args in CASES.items():
        make(name, *args)
