"""Helpers of the FastGRNNBatchNorm tests: the fixtures of tests/golden/batchnorm/ (make_batchnorm_golden.py), the
model built from them, and fp64 torch oracles of the eval-mode cell."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "batchnorm")
HIDDEN = [256, 128, 128]
CLASSES = 12
DEV = torch.device("cuda:0")


def load(name):
    d = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    sd = {k[3:]: torch.from_numpy(np.array(v)) for k, v in d.items() if k.startswith("sd/")}
    return d, sd


def trained_state_dict():
    """The checkpoint's full state dict: the unique tensors plus the ``unrollRNN.RNNCell`` duplicates."""
    d, sd = load("trained")
    full = {}
    for k in d["keys"]:
        k = str(k)
        full[k] = sd[k.replace(".unrollRNN.RNNCell.", ".cell.")].clone()
    return d, full


def build_model(device, batch_first=False):
    from kws_amd import RNNClassifierModel
    m = RNNClassifierModel("FastGRNNBatchNorm", 64, 3, HIDDEN, [None] * 3, [None] * 3, [1.0] * 3, [1.0] * 3,
                           "sigmoid", "tanh", num_classes=CLASSES, batch_first=batch_first, device=device)
    return m


def _bn(sd, pre, v):
    """Eval-mode BatchNorm1d, unfolded: (v - mean) / sqrt(var + eps) * gamma + beta (eps = 1e-5)."""
    return (v - sd[pre + "running_mean"]) / torch.sqrt(sd[pre + "running_var"] + 1e-5) * sd[pre + "weight"] + \
        sd[pre + "bias"]


GATES = {"sigmoid": torch.sigmoid, "relu": torch.relu, "tanh": torch.tanh}


def cell_params(sd, prefix):
    return {k[len(prefix):]: v.double() for k, v in sd.items() if k.startswith(prefix)}


@torch.no_grad()
def unfolded_scan(p, x, h0, gate="sigmoid"):
    """The reference cell's eval-mode formula (rnn.py:373-414) in fp64, step by step.  x [T,B,F] -> hs [T,B,H]."""
    h = h0.double()
    out = []
    for t in range(x.shape[0]):
        wc = _bn(p, "bn_w.", x[t].double() @ p["W"])
        uc = _bn(p, "bn_u.", h @ p["U"])
        z = GATES[gate](_bn(p, "bn_gate.", wc + uc + p["bias_gate"]))
        c = torch.tanh(_bn(p, "bn_update.", wc + uc + p["bias_update"]))
        h = z * h + (torch.sigmoid(p["zeta"]) * (1.0 - z) + torch.sigmoid(p["nu"])) * c
        out.append(h)
    return torch.stack(out)


@torch.no_grad()
def folded_scan(w, u, bg, bu, sg, sc, zeta, nu, x, h0, gate="sigmoid"):
    """The affine cell fastgrnn_hip_forward_unroll_affine computes, in torch: w [H,F], u [H,H] ([out,in])."""
    h = h0
    out = []
    for t in range(x.shape[0]):
        pre = x[t] @ w.t() + h @ u.t()
        z = GATES[gate](sg * pre + bg)
        c = torch.tanh(sc * pre + bu)
        h = z * h + (torch.sigmoid(zeta) * (1.0 - z) + torch.sigmoid(nu)) * c
        out.append(h)
    return torch.stack(out)


def model_oracle(sd, x, gate="sigmoid"):
    """fp64 stack: per-layer h_T and the log-probs of the head on the top layer's last step."""
    rin = torch.as_tensor(x).double()
    hT = []
    for l, H in enumerate(HIDDEN):
        p = cell_params(sd, "rnn_list.%d.cell." % l)
        hs = unfolded_scan(p, rin, torch.zeros(rin.shape[1], H, dtype=torch.float64, device=rin.device), gate)
        hT.append(hs[-1])
        rin = hs
    logits = rin[-1] @ sd["hidden2keyword.weight"].double().t() + sd["hidden2keyword.bias"].double()
    return hT, torch.log_softmax(logits, dim=1)


# ---- random eval-mode cells of the GPU tests and their scans in torch ------------------------------------------------

def random_bn(F, H, gate, seed):
    """A cell with hostile statistics: negative gammas, running variances at 0 (a = gamma / sqrt(eps)), and bn_u
    scales spanning 10^4 within every 16 consecutive units."""
    from kws_amd import FastGRNNBatchNorm
    torch.manual_seed(seed)
    m = FastGRNNBatchNorm(F, H, gate_nonlinearity=gate, device=DEV)
    with torch.no_grad():
        m.cell.W.mul_(0.5 / F ** 0.5 / 0.1)
        m.cell.U.mul_((0.3 if gate == "sigmoid" else 0.05) / H ** 0.5 / 0.1)
        m.cell.zeta.fill_(0.8); m.cell.nu.fill_(-1.5)
        m.cell.bias_gate.normal_(0, 0.5); m.cell.bias_update.normal_(0, 0.5)
        for bn in (m.cell.bn_w, m.cell.bn_u, m.cell.bn_gate, m.cell.bn_update):
            bn.weight.copy_(torch.randn(H, device=DEV)); bn.bias.normal_(0, 0.3)
            bn.running_mean.normal_(0, 0.3); bn.running_var.uniform_(0.5, 2.0)
            bn.running_var[::11] = 0.0
        j = torch.arange(H, device=DEV) % 16
        span = 10.0 ** (4.0 * j / 15.0 - 2.0)                    # 1e-2 .. 1e2 inside every 16 units
        m.cell.bn_u.running_var.fill_(1.0 - 1e-5)
        m.cell.bn_u.weight.copy_(span * torch.where(j % 3 == 0, -1.0, 1.0))
        if gate != "sigmoid":
            m.cell.bn_u.weight.mul_(0.1)
        if gate == "relu":        # an unbounded gate (h grows like the product of the z's): keep z mostly below 1
            m.cell.bn_w.running_var.uniform_(0.5, 2.0)
            m.cell.bn_gate.running_var.uniform_(0.5, 2.0)
            m.cell.bn_gate.weight.normal_(0, 0.1); m.cell.bn_gate.bias.fill_(-1.0)
    return m.eval()


def fp64_scan(m, x_tm, h0):
    from kws_amd import fold_batchnorm
    w, u, bg, bu, sg, sc = fold_batchnorm(m.cell.double())
    out = folded_scan(w, u, bg, bu, sg, sc, m.cell.zeta.reshape(()), m.cell.nu.reshape(()), x_tm.double(),
                        h0.double(), m.cell._gate_nonlinearity)
    m.cell.float()
    return out


def fp32_scan(m, x_tm, h0):
    from kws_amd import fold_batchnorm
    w, u, bg, bu, sg, sc = fold_batchnorm(m.cell)
    return folded_scan(w, u, bg, bu, sg, sc, m.cell.zeta.reshape(()), m.cell.nu.reshape(()), x_tm, h0,
                         m.cell._gate_nonlinearity)
