"""Classifier head on the last hidden state behind the C ABI's ``fastgrnn_hip_head_xent``.

The reference chains three torch modules after the last FastGRNN layer -- ``hidden2keyword = nn.Linear(H, C)``
on ``hs[T-1]`` (model.py:86-88, 226-227), ``F.log_softmax(dim=1)`` (model.py:229-230) and ``nn.NLLLoss()``
(trainClassifier.py:154,236) -- i.e. about eight small launches per training step for forward and backward.
``keyword_loss`` does all of it, gradients included, in two launches; ``head_predict`` is the forward-only tail
(scores, argmax and the count of correct rows of ``batch_accuracy``, trainClassifier.py:54-65) and ``vote_windows`` the
detector's majority vote over consecutive windows (inferencetry.py:217-227); ``KeywordHead`` owns the ``Linear``
parameters under the reference's names so a ``RNNClassifierModel`` state dict loads unchanged
(``hidden2keyword.weight`` / ``.bias``).
"""
import torch
from torch import nn
from torch.autograd import Function

from . import _lib
from .fastgrnn_cuda import _call, _check_input, _ptr


def head_xent(h_last, weight, bias, labels, want_log_probs=False):
    """One fused pass: returns (loss[1], log_probs[B,C] or None, d_h_last[B,H], d_weight[C,H], d_bias[C]) for
    loss = NLLLoss(mean)(log_softmax(h_last @ weight.T + bias), labels)."""
    lib = _lib.load()
    for t, n in ((h_last, "h_last"), (weight, "weight"), (bias, "bias"), (labels, "labels")):
        _check_input(t, n)
    if h_last.dim() != 2 or weight.dim() != 2 or weight.shape[1] != h_last.shape[1] or bias.numel() != weight.shape[0]:
        raise RuntimeError("head_xent: h_last [B,H], weight [C,H], bias [C]")
    if labels.dtype != torch.int64 or labels.numel() != h_last.shape[0]:
        raise RuntimeError("head_xent: labels must be int64 [B]")
    if h_last.dtype != torch.float32 or weight.dtype != torch.float32 or bias.dtype != torch.float32:
        raise RuntimeError("head_xent: float32 operands")
    B, H = h_last.shape
    Cn = weight.shape[0]
    dev = h_last.device
    with torch.cuda.device(dev):
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        logp = torch.empty((B, Cn), dtype=torch.float32, device=dev) if want_log_probs else None
        d_h = torch.empty_like(h_last)
        d_w = torch.empty_like(weight)
        d_b = torch.empty(Cn, dtype=torch.float32, device=dev)
        nbytes = lib.fastgrnn_hip_head_workspace_bytes(B, H, Cn)
        _call(lib.fastgrnn_hip_head_xent, "fastgrnn head_xent", None, dev, nbytes, B, H, Cn, _ptr(h_last), _ptr(weight),
              _ptr(bias), _ptr(labels), _ptr(loss), _ptr(logp), _ptr(d_h), _ptr(d_w), _ptr(d_b))
    return loss, logp, d_h, d_w, d_b


def head_predict(h_last, weight, bias, labels=None, want_log_probs=True):
    """The inference head in one call (``fastgrnn_hip_head_predict``): returns ``(pred, log_probs or None, n_correct or
    None)`` -- ``pred:[B]`` int32, the argmax of ``h_last @ weight.T + bias`` by ``torch.argmax``'s rules;
    ``log_probs:[B,C]``, the bits ``head_xent`` writes; with ``labels`` (int64 ``[B]``) ``n_correct:[1]`` int32, the
    number of rows with ``pred == labels`` (trainClassifier.py:54-65; a label of -100 never matches).  All three stay on
    the device and nothing synchronises."""
    lib = _lib.load()
    for t, n in ((h_last, "h_last"), (weight, "weight"), (bias, "bias")) + (((labels, "labels"),) if labels is not None else ()):
        _check_input(t, n)
    if h_last.dim() != 2 or weight.dim() != 2 or weight.shape[1] != h_last.shape[1] or bias.numel() != weight.shape[0]:
        raise RuntimeError("head_predict: h_last [B,H], weight [C,H], bias [C]")
    if labels is not None and (labels.dtype != torch.int64 or labels.numel() != h_last.shape[0]):
        raise RuntimeError("head_predict: labels must be int64 [B]")
    if h_last.dtype != torch.float32 or weight.dtype != torch.float32 or bias.dtype != torch.float32:
        raise RuntimeError("head_predict: float32 operands")
    B, H = h_last.shape
    Cn = weight.shape[0]
    dev = h_last.device
    with torch.cuda.device(dev):
        pred = torch.empty(B, dtype=torch.int32, device=dev)
        logp = torch.empty((B, Cn), dtype=torch.float32, device=dev) if want_log_probs else None
        n_correct = torch.empty(1, dtype=torch.int32, device=dev) if labels is not None else None
        nbytes = lib.fastgrnn_hip_head_predict_workspace_bytes(B, H, Cn) if labels is not None else 0
        _call(lib.fastgrnn_hip_head_predict, "fastgrnn head_predict", None, dev, nbytes, B, H, Cn, _ptr(h_last),
              _ptr(weight), _ptr(bias), _ptr(labels), _ptr(logp), _ptr(pred), _ptr(n_correct))
    return pred, logp, n_correct


def vote_windows(pred, num_windows=10, majority=5):
    """The reference detector's majority vote (inferencetry.py:217-227) over ``pred:[S,Nw]`` int32 window predictions of
    ``S`` independent streams (``fastgrnn_hip_vote_windows``): returns ``(majority, event)``, both ``[S,Nw]`` int32 on the
    device.  ``majority[s,w]`` is the most common of the last ``num_windows`` predictions up to window ``w`` if it has at
    least ``majority`` votes (ties: the value that entered the list first), else -1; ``event[s,w]`` is that value where
    the reference reports a detection -- it differs from the last one reported -- else -1."""
    lib = _lib.load()
    _check_input(pred, "pred")
    if pred.dim() != 2 or pred.dtype != torch.int32:
        raise RuntimeError("vote_windows: pred must be int32 [S,Nw]")
    S, Nw = pred.shape
    dev = pred.device
    with torch.cuda.device(dev):
        maj = torch.empty_like(pred)
        event = torch.empty_like(pred)
        _call(lib.fastgrnn_hip_vote_windows, "fastgrnn vote_windows", None, dev, None, S, Nw, int(num_windows),
              int(majority), _ptr(pred), _ptr(maj), _ptr(event))
    return maj, event


class KeywordLossFunction(Function):
    """loss = NLLLoss()(log_softmax(Linear(h_last)), labels); the gradients are computed with the forward (the
    loss is always differentiated in training) and scaled by the incoming grad in backward."""

    @staticmethod
    def forward(ctx, h_last, weight, bias, labels):
        loss, _, d_h, d_w, d_b = head_xent(h_last.contiguous(), weight.contiguous(), bias.contiguous(),
                                           labels.contiguous())
        ctx.save_for_backward(d_h, d_w, d_b)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, grad_loss):
        d_h, d_w, d_b = ctx.saved_tensors
        return d_h * grad_loss, d_w * grad_loss, d_b * grad_loss, None


def keyword_loss(h_last, weight, bias, labels):
    return KeywordLossFunction.apply(h_last, weight, bias, labels)


class KeywordHead(nn.Module):
    """``hidden2keyword`` (model.py:86-88) + log_softmax + NLLLoss.  ``forward(h_last)`` gives the reference's
    ``keyword_scores`` (log-probabilities, model.py:226-230, plain torch); ``loss(h_last, labels)`` the fused
    training loss (trainClassifier.py:236); ``predict(h_last)`` scores and argmax from the fused inference head."""

    def __init__(self, hidden_size, num_classes, device=None):
        super().__init__()
        self.hidden2keyword = nn.Linear(hidden_size, num_classes, device=device)

    def forward(self, h_last):
        return torch.log_softmax(self.hidden2keyword(h_last), dim=1)

    def loss(self, h_last, labels):
        return keyword_loss(h_last, self.hidden2keyword.weight, self.hidden2keyword.bias, labels)

    @torch.no_grad()
    def predict(self, h_last):
        """``(pred, log_probs)``: ``forward``'s scores and their argmax (int32) from the fused inference head."""
        pred, logp, _ = head_predict(h_last.contiguous(), self.hidden2keyword.weight.contiguous(),
                                     self.hidden2keyword.bias.contiguous())
        return pred, logp
