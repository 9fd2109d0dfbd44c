#!/usr/bin/env python3
"""Generate the BatchNorm keyword-spotter fixtures by running the REFERENCE's own BatchNorm cell.

Run in the build container only (needs /root/reference, read-only):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/batchnorm/make_batchnorm_golden.py

Writes DATA only, next to this script (a subdirectory: tests/conftest.py feeds every top-level
tests/golden/*.npz to the single-layer fixtures, whose schema these files do not follow):

* trained.npz -- the trained model model_batchnorm/FastGRNNBatchNorm_KeywordSpotter.pt: its unique tensors under the
  reference's key names (``rnn_list.{l}.cell.*``, ``hidden2keyword.*``; the ``unrollRNN.RNNCell`` duplicates are
  equal and listed in ``keys`` only), the checkpoint's full key list, a synthetic normalised input (time-major:
  the reference's batch_first head reads the last UTTERANCE, model.py:225-227), and the reference cell's eval-mode
  outputs in fp32 and in fp64 (the same cells converted with ``.double()``): per-layer h_T, the log-probs, and
  the fp32 error per layer.
* random_h100_f64.npz -- one cell with random BatchNorm statistics (negative gammas, running variances near 0) at
  H = 100, F = 24, nonzero h0, fp64: the full hidden-state sequence.
"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
sys.path.insert(0, "/root/reference")
import rnn  # noqa: E402  (the reference)

HERE = os.path.dirname(os.path.abspath(__file__))
CKPT = "/root/reference/model_batchnorm/FastGRNNBatchNorm_KeywordSpotter.pt"


def run_layer(cell, x, h0):
    """BaseRNN's per-timestep loop (rnn.py:588-668), eval mode."""
    h = h0
    hs = []
    for t in range(x.shape[0]):
        h = cell(x[t], h, training=False)
        hs.append(h)
    return torch.stack(hs)


def trained():
    sd = torch.load(CKPT, map_location="cpu", weights_only=False)["model_state_dict"]
    keys = list(sd.keys())
    layers = sorted({int(k.split(".")[1]) for k in keys if k.startswith("rnn_list.")})
    cells = []
    for l in layers:
        W = sd["rnn_list.%d.cell.W" % l]
        cell = rnn.FastGRNNBatchNormCell(W.shape[0], W.shape[1], gate_nonlinearity="sigmoid",
                                         update_nonlinearity="tanh")
        pre = "rnn_list.%d.cell." % l
        cell.load_state_dict({k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}, strict=True)
        cell.eval()
        cells.append(cell)
    fc_w, fc_b = sd["hidden2keyword.weight"], sd["hidden2keyword.bias"]
    T, B, F = 99, 8, cells[0].W.shape[0]
    g = torch.Generator().manual_seed(7)
    x = torch.randn(T, B, F, generator=g)                     # normalised MFCC frames: zero mean, unit variance
    out = {}
    for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
        rin = x.to(dt)
        with torch.no_grad():
            for l, cell in enumerate(cells):
                c = cell.to(dt)
                hs = run_layer(c, rin, torch.zeros(B, c.W.shape[1], dtype=dt))
                out["%s_h%d" % (tag, l)] = hs[-1].numpy()
                rin = hs
            logits = rin[-1] @ fc_w.to(dt).t() + fc_b.to(dt)
            out["%s_logp" % tag] = torch.log_softmax(logits, dim=1).numpy()
    for l in range(len(cells)):
        out["err_h%d" % l] = np.float64(np.abs(out["f32_h%d" % l] - out["f64_h%d" % l]).max())
    out["err_logp"] = np.float64(np.abs(out["f32_logp"] - out["f64_logp"]).max())
    data = {k: v.numpy() for k, v in sd.items() if not k.startswith("rnn_list.") or ".cell." in k}
    np.savez_compressed(os.path.join(HERE, "trained.npz"), keys=np.array(keys), x=x.numpy(),
                        meta_gate=np.array("sigmoid"), meta_update=np.array("tanh"),
                        **{"sd/" + k: v for k, v in data.items()}, **out)
    print("trained: layers %s, fp32 errors %s, logp %.3g" % (
        [tuple(c.W.shape) for c in cells], [float(out["err_h%d" % l]) for l in range(len(cells))],
        float(out["err_logp"])))


def random_h100():
    torch.manual_seed(11)
    T, B, F, H = 20, 5, 24, 100
    cell = rnn.FastGRNNBatchNormCell(F, H, gate_nonlinearity="sigmoid", update_nonlinearity="tanh").double()
    with torch.no_grad():
        cell.zeta.fill_(0.7); cell.nu.fill_(-2.5)
        cell.bias_gate.normal_(0, 0.5); cell.bias_update.normal_(0, 0.5)
        for bn in (cell.bn_w, cell.bn_u, cell.bn_gate, cell.bn_update):
            bn.weight.copy_(torch.randn(H, dtype=torch.float64) * 1.5)        # about a third negative
            bn.bias.normal_(0, 0.3)
            bn.running_mean.normal_(0, 0.5)
            bn.running_var.copy_(torch.rand(H, dtype=torch.float64) * 2.0)
            bn.running_var[::9] = 1e-40                                        # a = gamma / sqrt(eps)
    cell.eval()
    x = torch.randn(T, B, F, dtype=torch.float64)
    h0 = 0.5 * torch.randn(B, H, dtype=torch.float64)
    with torch.no_grad():
        hs = run_layer(cell, x, h0)
    sd = {k: v.numpy() for k, v in cell.state_dict().items()}
    np.savez_compressed(os.path.join(HERE, "random_h100_f64.npz"), x=x.numpy(), h0=h0.numpy(), hs=hs.numpy(),
                        meta_gate=np.array("sigmoid"), meta_update=np.array("tanh"),
                        **{"sd/" + k: v for k, v in sd.items()})
    print("random_h100_f64: max|hs| %.3g" % float(hs.abs().max()))


if __name__ == "__main__":
    trained()
    random_h100()
