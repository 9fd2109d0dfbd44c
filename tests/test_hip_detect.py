"""The inference tail on the GPU: fastgrnn_hip_head_predict (scores, argmax, count of correct rows), fastgrnn_hip_vote_windows
(the detector's majority vote) and the model methods built on them (predict, batch_accuracy, evaluate, detect_stream).

Operands, the fp64 reference and the plain-Python vote come from tests/detect_cases.py, computed once per session.
Bounds: log_probs within 1e-5 of the largest element, as tests/test_hip_parity.py holds the training head's; pred may
differ from the fp64 argmax only on rows whose fp64 top-two logit gap is below 2e-5 of the largest logit magnitude
(with the seeds of detect_cases there is no such row, asserted in tests/test_detect_cpu.py); integers are exact.
"""
import pytest
import torch

from tests import detect_cases as D

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from kws_amd import RNNClassifierModel, head
    from kws_amd.head import KeywordHead
DEV = torch.device("cuda:0")


def _dev(c):
    return c["h"].to(DEV), c["w"].to(DEV), c["b"].to(DEV), c["y"].to(DEV)


# ---- head_predict ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,Cn", D.HEAD_SHAPES)
def test_head_predict_vs_torch_fp64(B, H, Cn):
    c = D.head_case(B, H, Cn)
    h, w, b, y = _dev(c)
    pred, logp, n = head.head_predict(h, w, b, y)
    assert pred.dtype == torch.int32 and pred.shape == (B,) and logp.shape == (B, Cn) and n.dtype == torch.int32
    pred_c, logp_c = pred.cpu().long(), logp.cpu()
    ref = c["logp64"].float()
    err = float((logp_c - ref).abs().max()) / max(1e-30, float(ref.abs().max()))
    differ = pred_c != c["argmax64"]
    print("head_predict %s: log_probs err %.3g, pred differs on %d rows, excused %d, n_correct %d"
          % ((B, H, Cn), err, int(differ.sum()), int(c["excused"].sum()), int(n)))
    assert err <= 1e-5
    assert not bool((differ & ~c["excused"]).any())
    assert int(c["excused"].sum()) <= 0.01 * B
    assert int(n) == int((pred_c == c["y"]).sum())
    # self-consistency: the predicted class holds the row's largest score
    assert torch.equal(logp_c.gather(1, pred_c[:, None])[:, 0], logp_c.max(dim=1).values)
    # optional outputs change nothing else
    pred2, logp2, n2 = head.head_predict(h, w, b, y, want_log_probs=False)
    assert logp2 is None and torch.equal(pred2, pred) and torch.equal(n2, n)
    pred3, logp3, n3 = head.head_predict(h, w, b)
    assert n3 is None and torch.equal(pred3, pred) and torch.equal(logp3, logp)
    # twice the same bits
    again = head.head_predict(h, w, b, y)
    assert all(torch.equal(a, o) for a, o in zip(again, (pred, logp, n)))


@pytest.mark.parametrize("B,H,Cn", [(37, 128, 12), (33, 256, 64)])
def test_head_predict_scores_are_head_xents_bits(B, H, Cn):
    h, w, b, y = _dev(D.head_case(B, H, Cn))
    y = y.clamp(min=0)                                           # (head_xent's loss is not the subject: valid labels)
    _, logp, _ = head.head_predict(h, w, b, y)
    _, logp_x, _, _, _ = head.head_xent(h, w, b, y, want_log_probs=True)
    assert torch.equal(logp, logp_x)


@pytest.mark.parametrize("B,H,Cn", [s for s in D.HEAD_SHAPES if s[2] > 7])
def test_head_predict_exact_ties_go_to_the_lowest_index(B, H, Cn):
    """Class rows 3 and 7 of W and b are identical: their logits are the same bits, and the lower index wins."""
    c = D.head_case(B, H, Cn, tie=True)
    h, w, b, _ = _dev(c)
    pred = head.head_predict(h, w, b)[0].cpu().long()
    rows = c["argmax64"] == 3
    assert int(rows.sum()) >= 1 and bool((pred[rows] == 3).all())
    assert not bool((pred == 7).any())


def test_head_predict_nan_counts_as_the_maximum():
    c = D.head_case(37, 128, 12)
    h, w, b, _ = _dev(c)
    pred0, logp0, _ = head.head_predict(h, w, b)
    hn = h.clone()
    hn[21, 5] = float("nan")
    pred, logp, _ = head.head_predict(hn, w, b)
    assert int(pred[21]) == int(torch.argmax(logp[21]))          # (every score of the row is NaN: the first one)
    keep = torch.arange(37, device=DEV) != 21
    assert torch.equal(pred[keep], pred0[keep]) and torch.equal(logp[keep], logp0[keep])
    # NaN logits in classes 5 and 9 only: the first NaN is the argmax of the logits on every row
    bn = b.clone()
    bn[5] = bn[9] = float("nan")
    assert bool((head.head_predict(h, w, bn, want_log_probs=False)[0] == 5).all())


def test_keyword_head_predict_is_its_forward():
    c = D.head_case(37, 128, 12)
    kh = KeywordHead(128, 12, device=DEV)
    with torch.no_grad():
        kh.hidden2keyword.weight.copy_(c["w"]); kh.hidden2keyword.bias.copy_(c["b"])
        pred, logp = kh.predict(c["h"].to(DEV))
        ref = kh(c["h"].to(DEV))
    assert float((logp - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
    assert torch.equal(pred.cpu().long(), c["argmax64"])


# ---- vote_windows ------------------------------------------------------------------------------------------------------
def _vote_matches(pred, K, M):
    maj, ev = head.vote_windows(pred.to(DEV), K, M)
    want_maj, want_ev = D.vote_reference_streams(pred.tolist(), K, M)
    assert maj.dtype == torch.int32 and maj.shape == pred.shape and ev.shape == pred.shape
    assert maj.cpu().tolist() == want_maj
    assert ev.cpu().tolist() == want_ev


@pytest.mark.parametrize("name", D.VOTE_CASES)
def test_vote_windows_equals_the_python_vote(name):
    pred, K, M = D.vote_case(name)
    _vote_matches(pred, K, M)


@pytest.mark.parametrize("case", D.TYPED_CASES, ids=[c[0] for c in D.TYPED_CASES])
def test_vote_windows_on_typed_out_cases(case):
    _, pred, K, M, majority, event = case
    maj, ev = head.vote_windows(torch.tensor([pred], dtype=torch.int32, device=DEV), K, M)
    assert maj.cpu().tolist() == [majority] and ev.cpu().tolist() == [event]


def test_vote_windows_streams_do_not_leak():
    pred, K, M = D.vote_case("leak")
    both = head.vote_windows(pred.to(DEV), K, M)
    alone = head.vote_windows(pred[1:].to(DEV).contiguous(), K, M)
    assert all(torch.equal(b[1:], a) for b, a in zip(both, alone))
    assert both[0][1, :4].cpu().tolist() == [-1] * 4


# ---- the model methods -------------------------------------------------------------------------------------------------
def _model(F, hidden, seed, Cn=12):
    torch.manual_seed(seed)
    n = len(hidden)
    return RNNClassifierModel("FastGRNNCUDA", F, n, hidden, [None] * n, [None] * n, [1.0] * n, [1.0] * n, "sigmoid", "tanh",
                              num_classes=Cn, device=DEV)


@pytest.mark.parametrize("F,hidden,S", [(32, [128], 2), (64, [256, 128], 1)])
def test_detect_stream_is_score_stream_plus_the_vote(F, hidden, S):
    m = _model(F, hidden, 6)
    stream = torch.randn(S, 140, F, generator=torch.Generator().manual_seed(12)).to(DEV)
    pred, maj, ev = m.detect_stream(stream, hop=3, window=99)
    scores = m.score_stream(stream, hop=3, window=99)
    nw = (140 - 99) // 3 + 1
    assert pred.shape == (S, nw) and pred.dtype == torch.int32 and scores.shape == (S, nw, 12)
    top2 = scores.topk(2, dim=-1).values
    assert int((top2[..., 0] == top2[..., 1]).sum()) == 0        # no exact score ties: the argmax is unambiguous
    assert torch.equal(pred.long(), scores.argmax(-1))
    want_maj, want_ev = D.vote_reference_streams(pred.cpu().tolist(), 10, 5)
    assert maj.cpu().tolist() == want_maj and ev.cpu().tolist() == want_ev
    assert m.hidden_states == [None] * len(hidden)               # neither read nor written, as in score_stream
    # other vote parameters reach the kernel
    _, maj3, ev3 = m.detect_stream(stream, hop=3, window=99, num_windows=3, majority=2)
    assert (maj3.cpu().tolist(), ev3.cpu().tolist()) == D.vote_reference_streams(pred.cpu().tolist(), 3, 2)


def test_predict_batch_accuracy_and_evaluate():
    T, B, F, Cn = 9, 37, 32, 12
    m, twin = _model(F, [256, 128], 7), _model(F, [256, 128], 7)
    g = torch.Generator().manual_seed(13)
    batches = [(torch.randn(T, B, F, generator=g).to(DEV), torch.randint(0, Cn, (B,), generator=g)) for _ in range(3)]
    x, y = batches[0]
    pred, logp = m.predict(x)
    with torch.no_grad():
        ref = twin(x)
    assert pred.dtype == torch.int32 and logp.shape == (B, Cn)
    assert float((logp - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
    assert torch.equal(pred.long(), logp.argmax(1))
    # the carried states are forward's (the same kernels under no_grad)
    assert len(m.hidden_states) == 2 and all(torch.equal(a, b) for a, b in zip(m.hidden_states, twin.hidden_states))
    # batch_accuracy: the reference's triple
    per_batch = []
    for xb, yb in batches:
        m.init_hidden()
        percent, passed, results = m.batch_accuracy(xb, yb)
        assert isinstance(passed, int) and len(results) == B and all(isinstance(r, int) for r in results)
        assert passed == sum(int(r == int(t)) for r, t in zip(results, yb))
        assert percent == float(passed) * 100.0 / float(B)
        per_batch.append(passed)
    m.init_hidden()
    assert m.batch_accuracy(x, y)[2] == pred.cpu().tolist()
    # labels that match: the count follows
    m.init_hidden()
    assert m.batch_accuracy(x, pred.long())[1] == B
    # evaluate: init_hidden per batch, counts added on the device
    m.train()
    assert m.evaluate(iter(batches)) == sum(per_batch) / (3 * B)
    assert not m.training                                        # (trainClassifier.py:290)


@pytest.mark.parametrize("H,Cn", [(128, 12), (256, 64)])         # the second: 86 KB of dynamic LDS, the opt-in attribute
def test_head_predict_then_vote_in_a_graph_replays_with_new_data(H, Cn):
    S, Nw = 2, 24
    g = torch.Generator().manual_seed(14)
    w, b = (0.3 * torch.randn(Cn, H, generator=g)).to(DEV), (0.1 * torch.randn(Cn, generator=g)).to(DEV)
    hs = [torch.randn(S * Nw, H, generator=g).to(DEV) for _ in range(3)]
    ys = [torch.randint(0, Cn, (S * Nw,), generator=g).to(DEV) for _ in range(3)]

    def step(h, y):
        pred, logp, n = head.head_predict(h, w, b, y)
        maj, ev = head.vote_windows(pred.reshape(S, Nw), 4, 2)
        return pred, logp, n, maj, ev

    want = [tuple(t.clone() for t in step(h, y)) for h, y in zip(hs, ys)]
    assert not torch.equal(want[1][0], want[2][0])
    h_in, y_in = hs[0].clone(), ys[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(h_in, y_in)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step(h_in, y_in)
    for k in (1, 2):
        h_in.copy_(hs[k]); y_in.copy_(ys[k])
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, e) for a, e in zip(out, want[k])), k
