"""fastgrnn_hip_forward_windows_train / fastgrnn_hip_backward_windows on the GPU: training on utterances that are windows
of a shared frame pool.

The pool is R = 300 rows cut from the middle of a larger buffer whose rows before and after are NaN.  Per shape and gate
four cases cover T in {1, 2, 7, 99}, B in {1, 16, 17, 33} (one workgroup, a ragged tail, more than two workgroups), four
sets of starts (hop 1 overlapping, all windows the same, descending, one holding both 0 and R - T), both layouts and a
dense / last-state gradient; which of them meet rotates with the gate.  h0 is non-zero.  Every case checks, on one call
of each C entry point into caller-owned buffers:
 (a) hs and the saved pre-activation are torch.equal to forward_unroll under FASTGRNN_FLAG_SAVE_PREACT on the gathered
     windows (the loop is unchanged; a row of the F = 64 frame GEMM does not depend on its position);
 (b) every gradient is torch.equal to backward_unroll on the gathered windows with d_x == NULL (SAVE_PREACT, and
     NO_INPUT_GRAD on H = 128): the same arithmetic and the same work partition;
 (c) hs and every gradient against the fp64 oracle on the gathered windows, under the bounds the existing suites apply
     to these shapes: hs max |hs - ref| / max(1, |ref|) <= 1e-5 (tests/test_hip_windows.py, tests/test_hip_parity.py),
     gradients tests/test_hip_parity.py::_check_grads at 2e-5 (tests/test_hip_no_input_grad.py compares bits and holds
     no oracle bound of its own).  relu gates are kept off the kink as tests/test_hip_parity.py does;
 (d) everything is finite with the NaN rows around the pool; the sentinels behind hs, saved, every gradient and the
     workspace (whose last bytes are the gathered copy of x) are intact; that copy alone is torch.equal to
     gather_windows.
The fp64 comparison over 99 steps needs a recurrence that does not amplify rounding differences: a relu or tanh gate
does not bound the state (tests/test_hip_parity.py keeps such cases to a few steps for that reason).  T = 99 is wanted
here for the addresses, so in the T = 99 cases of those two gates u is scaled by 0.25, which makes the recurrence
contractive; the bounds are the same.  (With the unscaled u of the shorter cases the relu state overflows fp32 before
step 99 on H = 256 and the tanh-gated scan is 7e-3 / 0.3 from the oracle in the existing forward as well: (a) and (b)
held bit for bit there.)
Then the modules: unroll_windows against forward(gather_windows(...)), the low-rank fallback, and loss_windows against
loss() on the gathered batch for a 64 -> 256 -> 128 model at B = 33, T = 99.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from kws_amd import FastGRNNCUDA, RNNClassifierModel, _lib, fastgrnn_cuda
from kws_amd.rnn import gather_windows
from tests import layer_cases as LC
from tests import support as S

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SP, BM, GL, NIG = _lib.FLAG_SAVE_PREACT, _lib.FLAG_BATCH_MAJOR, _lib.FLAG_GRAD_LAST, _lib.FLAG_NO_INPUT_GRAD
GATES = ("sigmoid", "relu", "tanh")
SHAPES = [(128, 32), (256, 32), (256, 64)]
R, PAD = 300, 128
SENTINEL = -7777.0
GRADS = ["d_bias_gate", "d_bias_update", "d_zeta", "d_nu", "d_h0", "d_w", "d_u"]
TB = [(99, 33), (7, 17), (2, 16), (1, 1)]
KINDS = ["hop1", "desc", "ends", "same"]


def _cases():
    """(H, F, gate, T, B, kind, batch_major, grad_last): four per shape and gate, the pairing rotating with the gate
    (B = 1 never meets "ends", which needs two windows)."""
    out = []
    for H, F in SHAPES:
        for g, gate in enumerate(GATES):
            for i, (T, B) in enumerate(TB):
                out.append((H, F, gate, T, B, KINDS[(i + g) % 4], bool((i + g) % 2), bool(((i + g) // 2) % 2)))
    return out


CASES = _cases()


def _id(c):
    H, F, gate, T, B, kind, bm, gl = c
    return "H%dF%d-%s-T%dB%d-%s-%s-%s" % (H, F, gate, T, B, kind, "bm" if bm else "tm", "last" if gl else "dense")


def test_the_cases_cover_every_axis_per_shape_and_gate():
    for H, F in SHAPES:
        for gate in GATES:
            mine = [c for c in CASES if c[:3] == (H, F, gate)]
            assert {c[3] for c in mine} == {1, 2, 7, 99} and {c[4] for c in mine} == {1, 16, 17, 33}
            assert {c[5] for c in mine} == set(KINDS)
            assert {c[6] for c in mine} == {False, True} and {c[7] for c in mine} == {False, True}
            assert not any(c[4] == 1 and c[5] == "ends" for c in mine)


@functools.lru_cache(maxsize=None)
def _buffer(F):
    """The pool's R rows in the middle of a larger buffer, NaN before and after."""
    g = torch.Generator().manual_seed(2000 + F)
    buf = torch.full((PAD + R + PAD, F), float("nan"))
    buf[PAD:PAD + R] = torch.randn(R, F, generator=g)
    return buf.to(DEV)


def _pool(F):
    return _buffer(F)[PAD:PAD + R]


@functools.lru_cache(maxsize=None)
def _starts(kind, B, T):
    last = R - T
    if kind == "hop1":
        s = torch.arange(B)
    elif kind == "same":
        s = torch.full((B,), min(57, last))
    elif kind == "desc":
        s = last - torch.arange(B) * (last // B)
    else:
        g = torch.Generator().manual_seed(7 * B + T)
        s = torch.randint(0, last + 1, (B,), generator=g)
        s[0], s[B - 1] = last, 0                  # both ends; the second one in the ragged tile where there is one
    assert int(s.min()) >= 0 and int(s.max()) <= last
    if kind in ("desc", "ends"):
        assert int(s.max()) == last
    if kind == "ends":
        assert int(s.min()) == 0
    return s.to(torch.int32).to(DEV)


@functools.lru_cache(maxsize=None)
def _h0(B, H):
    g = torch.Generator().manual_seed(B + H)
    return (0.5 * torch.randn(B, H, generator=g)).to(DEV)


@functools.lru_cache(maxsize=None)
def _problem(H, F, gate, T, B, kind, gl):
    """Everything a case shares whatever its layout, computed once: parameters (numpy and device), the gathered
    windows [T,B,F], the gradient in time-major form, and the fp64 oracle's hs and gradients."""
    p, _ = LC.plain_cell(H, F, gate)
    x = gather_windows(_pool(F), _starts(kind, B, T), T).transpose(0, 1).contiguous()
    h0 = _h0(B, H)
    xn, hn = x.cpu().numpy(), h0.cpu().numpy()
    if T == 99 and gate != "sigmoid":              # a contractive recurrence for the 99-step comparison (docstring)
        p = dict(p)
        p["u"] = (0.25 * p["u"]).astype(np.float32)
    if gate == "relu":
        p = S.keep_relu_gates_off_the_kink(p, xn, hn)
    P = S.cell_tensors(p)
    g = torch.Generator().manual_seed(T * 1000 + B)
    G = torch.randn(T, B, H, generator=g)
    if gl:
        G[:-1] = 0.0
    hs_o, _, _, g_o = S.oracle64(xn, G.numpy(), p, hn, gate)
    g_o.pop("d_x")
    return P, x, G.to(DEV), hs_o, g_o


def _ptr(t):
    return C.c_void_p(None if t is None else t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _with_tail(shape, dtype=torch.float32):
    """A sentinel-filled buffer with room for `shape` plus a trailing block of 64 elements; (view, tail)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 64,), SENTINEL, dtype=dtype, device=DEV)
    return buf[:n].view(shape), buf[n:]


def _raw_forward(H, F, gate, flags, pool, starts, T, h0, P, hs, saved):
    lib = _lib.load()
    d = _lib.Desc(T, starts.numel(), F, H, 0, 0, S.NONLINEARITY[gate], 2, _lib.F32, flags)
    assert lib.fastgrnn_hip_train_windows_supported(C.byref(d)) == 1
    nbytes = int(lib.fastgrnn_hip_train_windows_forward_workspace_bytes(C.byref(d), R))
    ws = torch.full((nbytes + 256,), 0x5A, dtype=torch.uint8, device=DEV)
    prm = _lib.Params(_ptr(P["w"]), _ptr(P["u"]), None, None, None, None, _ptr(P["bias_gate"]), _ptr(P["bias_update"]),
                      _ptr(P["zeta"]), _ptr(P["nu"]))
    st = lib.fastgrnn_hip_forward_windows_train(C.byref(d), C.byref(prm), _ptr(pool), R, _ptr(starts), _ptr(h0),
                                                _ptr(hs), _ptr(saved), _ptr(ws) if nbytes else None, nbytes, _stream())
    assert st == 0, _lib.status_string(st)
    torch.cuda.synchronize()
    assert bool((ws[nbytes:] == 0x5A).all()), "wrote beyond the forward's workspace"


def _raw_backward(H, F, gate, flags, pool, starts, T, h0, P, G, hs, saved):
    """-> ({name: gradient}, their sentinel tails, the workspace, the bytes the library asked for)"""
    lib = _lib.load()
    B = starts.numel()
    d = _lib.Desc(T, B, F, H, 0, 0, S.NONLINEARITY[gate], 2, _lib.F32, flags)
    assert lib.fastgrnn_hip_train_windows_supported(C.byref(d)) == 1
    nbytes = int(lib.fastgrnn_hip_train_windows_backward_workspace_bytes(C.byref(d), R))
    ws = torch.full((nbytes + 256,), 0x5A, dtype=torch.uint8, device=DEV)
    shapes = {"d_bias_gate": (1, H), "d_bias_update": (1, H), "d_zeta": (1, 1), "d_nu": (1, 1), "d_h0": (B, H),
              "d_w": (H, F), "d_u": (H, H)}
    out, tails = {}, {}
    for k in GRADS:
        out[k], tails[k] = _with_tail(shapes[k])
    prm = _lib.Params(_ptr(P["w"]), _ptr(P["u"]), None, None, None, None, _ptr(P["bias_gate"]), _ptr(P["bias_update"]),
                      _ptr(P["zeta"]), _ptr(P["nu"]))
    grads = _lib.Grads(None, _ptr(out["d_bias_gate"]), _ptr(out["d_bias_update"]), _ptr(out["d_zeta"]),
                       _ptr(out["d_nu"]), _ptr(out["d_h0"]), _ptr(out["d_w"]), _ptr(out["d_u"]), None, None, None, None)
    st = lib.fastgrnn_hip_backward_windows(C.byref(d), C.byref(prm), _ptr(G), _ptr(pool), R, _ptr(starts), _ptr(hs),
                                           _ptr(saved), _ptr(h0), C.byref(grads), _ptr(ws), nbytes, _stream())
    assert st == 0, _lib.status_string(st)
    torch.cuda.synchronize()
    return out, tails, ws, nbytes


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_train_windows_vs_existing_calls_oracle_and_sentinels(case):
    H, F, gate, T, B, kind, bm, gl = case
    P, x_tm, G_tm, hs_o, g_o = _problem(H, F, gate, T, B, kind, gl)
    pool, starts, h0 = _pool(F), _starts(kind, B, T), _h0(B, H)
    layout = BM if bm else 0
    lay = (lambda t: t.transpose(0, 1).contiguous()) if bm else (lambda t: t)     # [T,B,.] -> the case's layout
    assert bool(torch.isnan(_buffer(F)[:PAD]).all()) and bool(torch.isnan(_buffer(F)[PAD + R:]).all())

    # ---- forward: into caller-owned hs / saved with sentinel tails
    shape = (B, T, H) if bm else (T, B, H)
    hs, hs_tail = _with_tail(shape)
    saved, saved_tail = _with_tail(shape)
    _raw_forward(H, F, gate, layout, pool, starts, T, h0, P, hs, saved)
    assert bool((hs_tail == SENTINEL).all()) and bool((saved_tail == SENTINEL).all()), "wrote beyond hs / saved"
    assert bool(torch.isfinite(hs).all()) and bool(torch.isfinite(saved).all()), "not finite: read beyond the pool?"
    # (a) the existing forward on the gathered windows: the same bits
    x = lay(x_tm)
    want_hs, want_pre = S.forward_unroll(x, h0, P, gate, flags=SP | layout)[:2]
    assert torch.equal(hs, want_hs), "hs differs from forward_unroll on the gathered windows"
    assert torch.equal(saved, want_pre), "the saved pre-activation differs from forward_unroll's"

    # ---- backward
    G = (G_tm[-1] if gl else lay(G_tm)).contiguous()
    got, tails, ws, nbytes = _raw_backward(H, F, gate, layout | (GL if gl else 0), pool, starts, T, h0, P, G, hs, saved)
    for k in GRADS:
        assert bool((tails[k] == SENTINEL).all()), "wrote beyond " + k
        assert bool(torch.isfinite(got[k]).all()), k
    assert bool((ws[nbytes:] == 0x5A).all()), "wrote beyond the workspace (its end is the gathered copy of x)"
    # (d) the gathered copy alone: the last align256(T*B*F*4) bytes of the workspace
    copy_bytes = (T * B * F * 4 + 255) // 256 * 256
    d0 = _lib.Desc(T, B, F, H, 0, 0, S.NONLINEARITY[gate], 2, _lib.F32, layout | (GL if gl else 0))
    assert nbytes == int(_lib.load().fastgrnn_hip_backward_workspace_bytes(C.byref(d0))) + copy_bytes
    copy = ws[nbytes - copy_bytes:nbytes - copy_bytes + T * B * F * 4].view(torch.float32).view(x.shape)
    assert torch.equal(copy, x), "the gather kernel's copy differs from gather_windows"
    assert bool((ws[nbytes - copy_bytes + T * B * F * 4:nbytes] == 0x5A).all())
    # (b) the existing backward on the gathered windows without d_x: the same bits
    ref = S.backward_of((want_hs, want_pre), G, x, h0, P, gate, flags=SP | layout | (GL if gl else 0), biases=True,
                        need_dx=False)
    torch.cuda.synchronize()
    assert ref[0].numel() == 0
    for k, v in zip(GRADS, ref[1:8]):
        assert got[k].shape == v.shape and torch.equal(got[k], v), \
            (k, float((got[k] - v).abs().max()), "differs from backward_unroll on the gathered windows")
    # the pool and its surroundings are untouched
    assert bool(torch.isnan(_buffer(F)[:PAD]).all()) and bool(torch.isnan(_buffer(F)[PAD + R:]).all())

    # (c) the fp64 oracle
    hs_tm = (hs.transpose(0, 1) if bm else hs).cpu().numpy()
    err = float((np.abs(hs_tm - hs_o) / np.maximum(1.0, np.abs(hs_o))).max())
    gerr = {k: float(np.abs(got[k].cpu().numpy().reshape(g_o[k].shape) - g_o[k]).max() / max(1.0, np.abs(g_o[k]).max()))
            for k in GRADS}
    print("%s: hs %.3g (bound 1e-5); gradients %s (bound 2e-5, d_zeta / d_nu also 2e-7 of their terms' magnitudes)"
          % (_id(case), err, " ".join("%s %.3g" % kv for kv in gerr.items())))
    assert err <= 1e-5
    S.check_grads({k: got[k] for k in GRADS}, g_o, tol=2e-5, scalar_term_tol=S.SCALAR_TERM_TOL, tag=_id(case))


# ---- modules -----------------------------------------------------------------------------------------------------------

def _module_grads(m, run, h0):
    for q in m.parameters():
        q.grad = None
    h = h0.clone().requires_grad_(True)
    out = run(h)
    out.sum().backward()
    torch.cuda.synchronize()
    return out.detach().clone(), [q.grad.clone() for q in m.parameters()], h.grad.clone()


@pytest.mark.parametrize("H,F,batch_first,last_state", [(128, 32, False, False), (128, 32, True, True),
                                                        (256, 32, True, False), (256, 64, False, True)],
                         ids=["h128-tm", "h128-bm-last", "h256f32-bm", "h256f64-tm-last"])
def test_unroll_windows_equals_forward_on_gathered_windows(H, F, batch_first, last_state):
    T, B = 7, 17
    torch.manual_seed(H + F)
    m = FastGRNNCUDA(F, H, batch_first=batch_first, device=DEV)
    pool, starts, h0 = _pool(F), _starts("ends", B, T), _h0(B, H)
    assert fastgrnn_cuda.train_windows_supported(T, B, F, H, flags=(BM if batch_first else 0) | (GL if last_state else 0))
    w = gather_windows(pool, starts, T)
    x = w if batch_first else w.transpose(0, 1).contiguous()
    want = _module_grads(m, lambda h: m(x, hiddenState=h, last_state=last_state), h0)
    for st in (starts, starts.long()):
        got = _module_grads(m, lambda h: m.unroll_windows(pool, st, T, hiddenState=h, last_state=last_state), h0)
        assert got[0].shape == want[0].shape and torch.equal(got[0], want[0])
        for (name, _), a, b in zip(m.named_parameters(), got[1], want[1]):
            assert torch.equal(a, b), name
        assert torch.equal(got[2], want[2]), "hiddenState gradient"
    # without a graph: the same call, the same bits
    with torch.no_grad():
        out = m.unroll_windows(pool, starts, T, hiddenState=h0, last_state=last_state)
    assert not out.requires_grad and torch.equal(out, want[0])
    bad = starts.clone()
    bad[3] = R - T + 1
    with pytest.raises(ValueError):
        m.unroll_windows(pool, bad, T)
    with pytest.raises(ValueError):
        m.unroll_windows(pool.clone().requires_grad_(True), starts, T)


def test_lowrank_cell_falls_back_to_gathered_windows():
    T, B = 7, 17
    torch.manual_seed(3)
    m = FastGRNNCUDA(32, 256, wRank=8, uRank=8, device=DEV)
    assert not fastgrnn_cuda.train_windows_supported(T, B, 32, 256, w_rank=8, u_rank=8)
    pool, starts, h0 = _pool(32), _starts("desc", B, T), _h0(B, 256)
    x = gather_windows(pool, starts, T).transpose(0, 1).contiguous()
    for last in (False, True):
        want = _module_grads(m, lambda h: m(x, hiddenState=h, last_state=last), h0)
        got = _module_grads(m, lambda h: m.unroll_windows(pool, starts, T, hiddenState=h, last_state=last), h0)
        assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[2])
        for a, b in zip(got[1], want[1]):
            assert torch.equal(a, b)


def test_loss_windows_equals_loss_on_the_gathered_batch():
    T, B, F = 99, 33, 64
    torch.manual_seed(11)
    m = RNNClassifierModel("FastGRNNCUDA", F, 2, [256, 128], [None, None], [None, None], [1.0, 1.0], [1.0, 1.0],
                           "sigmoid", "tanh", num_classes=12, device=DEV)
    pool, starts = _pool(F), _starts("ends", B, T)
    labels = torch.randint(0, 12, (B,), generator=torch.Generator().manual_seed(4)).to(DEV)
    x = gather_windows(pool, starts, T).transpose(0, 1).contiguous()

    def two_steps(step):
        """Two steps, the second from the hidden states the first one carried over."""
        m.init_hidden()
        out = []
        for _ in range(2):
            for q in m.parameters():
                q.grad = None
            loss = step()
            loss.backward()
            torch.cuda.synchronize()
            out.append((loss.detach().clone(), [q.grad.clone() for q in m.parameters()],
                        [h.clone() for h in m.hidden_states]))
        m.init_hidden()
        return out

    want = two_steps(lambda: m.loss(x, labels))
    got = two_steps(lambda: m.loss_windows(pool, starts, labels, window=T))
    for (la, ga, ha), (lb, gb, hb) in zip(got, want):
        assert torch.equal(la, lb), (float(la), float(lb))
        for (name, _), a, b in zip(m.named_parameters(), ga, gb):
            assert torch.equal(a, b), name
        for a, b in zip(ha, hb):
            assert torch.equal(a, b)
    assert not torch.equal(want[0][0], want[1][0])                           # the carried state took part
    with pytest.raises(ValueError):
        m.loss_windows(pool, starts + 1, labels, window=T)                    # R - T + 1 is out of range


def test_loss_windows_on_a_batchnorm_model_gathers_in_front_of_layer_0():
    """The BatchNorm families gather the windows and run loss(): the same loss, gradients and running statistics as
    loss() on the gathered batch, from the same initial state."""
    T, B, F = 7, 17, 32
    pool, starts = _pool(F), _starts("ends", B, T)
    labels = torch.randint(0, 12, (B,), generator=torch.Generator().manual_seed(5)).to(DEV)
    x = gather_windows(pool, starts, T).transpose(0, 1).contiguous()
    torch.manual_seed(3)
    m = RNNClassifierModel("FastGRNNBatchNormCUDA", F, 2, [128, 128], [None, None], [None, None], [1.0, 1.0],
                           [1.0, 1.0], "sigmoid", "tanh", num_classes=12, device=DEV).train()
    state = {k: v.clone() for k, v in m.state_dict().items()}

    def step(run):
        m.load_state_dict(state)
        m.init_hidden()
        for q in m.parameters():
            q.grad = None
        loss = run()
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach().clone(), [q.grad.clone() for q in m.parameters()], \
            {k: v.clone() for k, v in m.state_dict().items()}

    lb, gb, sb = step(lambda: m.loss(x, labels))
    la, ga, sa = step(lambda: m.loss_windows(pool, starts, labels, window=T))
    assert torch.equal(la, lb), (float(la), float(lb))
    for (name, _), a, b in zip(m.named_parameters(), ga, gb):
        assert torch.equal(a, b), name
    assert any(not torch.equal(sb[k], state[k]) for k in state)               # the running statistics moved ...
    for k in state:
        assert torch.equal(sa[k], sb[k]), k                                   # ... and the same way
    with pytest.raises(ValueError):
        m.loss_windows(pool, starts + 1, labels, window=T)
