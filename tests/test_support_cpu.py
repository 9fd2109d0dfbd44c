"""The shared checkers of tests/support.py, pinned on the CPU: the suite must not go green because a helper stopped
asserting, compared less than it says, or made another operator call than the one written at the call site."""
import numpy as np
import pytest
import torch

from kws_amd import fastgrnn_cuda
from oracle import fastgrnn_oracle as O
from tests import support as S


# ---- bits_equal / assert_same_bits ---------------------------------------------------------------------------------------

def _rejected(a, b):
    with pytest.raises(AssertionError):
        S.assert_same_bits(a, b, "pair")
    return not S.bits_equal(a, b)


def _accepted(a, b):
    S.assert_same_bits(a, b, "pair")
    return S.bits_equal(a, b)


def _next_up(t):
    """every element one unit in the last place further from zero"""
    i = {2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]
    return (t.contiguous().view(i) + 1).view(t.dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float64])
def test_bits_reject_one_ulp(dtype):
    a = torch.tensor([[1.0, -2.5, 3.0], [0.75, 1e-3, 100.0]]).to(dtype)
    assert _accepted(a, a.clone())
    b = a.clone()
    b[1, 2] = _next_up(a)[1, 2]
    assert float((a.double() - b.double()).abs().max()) > 0
    assert _rejected(a, b)


def test_bits_reject_signed_zero():
    a, b = torch.zeros(4), torch.zeros(4)
    b[2] = -0.0
    assert torch.equal(a, b)                    # equal as values
    assert _rejected(a, b)


def test_bits_reject_shape_mismatch_with_equal_bytes():
    a = torch.arange(6, dtype=torch.float32)
    assert _rejected(a.view(2, 3), a.view(3, 2))
    assert _rejected(a.view(1, 6), a)


def test_bits_reject_dtype_mismatch():
    a = torch.tensor([1.0, 2.0, -3.0])
    assert _rejected(a, a.double())             # equal values
    assert _rejected(a, a.view(torch.int32))    # equal bytes
    z = torch.zeros(4)
    assert _rejected(z.to(torch.bfloat16), z.to(torch.float16))


def test_bits_accept_equal_nan_payloads_and_tell_payloads_apart():
    quiet = torch.tensor([0x7FC00000, 0x7F800001, 0x3F800000], dtype=torch.int32).view(torch.float32)
    assert torch.isnan(quiet[:2]).all() and not torch.equal(quiet, quiet.clone())      # (NaN != NaN as values)
    assert _accepted(quiet, quiet.clone())
    other = torch.tensor([0x7FC00001, 0x7F800001, 0x3F800000], dtype=torch.int32).view(torch.float32)
    assert _rejected(quiet, other)


def test_bits_accept_a_non_contiguous_view_of_equal_values():
    a = torch.arange(24, dtype=torch.float32).reshape(2, 3, 4)
    view = a.permute(2, 0, 1)
    assert not view.is_contiguous()
    assert _accepted(view, view.contiguous())
    assert _accepted(a.to(torch.bfloat16).transpose(0, 1), a.to(torch.bfloat16).transpose(0, 1).contiguous())
    assert _accepted(torch.arange(5, dtype=torch.int32), torch.arange(5, dtype=torch.int32))    # integers as they are


# ---- check_grads ---------------------------------------------------------------------------------------------------------

def _ref(scale):
    """d_w with max|ref| = scale, d_zeta = scale, and the sums of d_zeta's / d_nu's term magnitudes"""
    return {"d_w": np.array([[scale, -0.5 * scale], [0.25 * scale, 0.0]]), "d_zeta": np.array([[scale]]),
            "d_nu": np.array([[-scale]]), "_abs_zeta": 1e4 * scale, "_abs_nu": 1e4 * scale}


def _off(ref, key, err, dtype=np.float32):
    """ref's gradients as ``dtype`` results, entry [0, 0] of ``key`` off by err"""
    got = {k: np.array(v, np.float64) for k, v in ref.items() if not k.startswith("_")}
    got[key][0, 0] += err
    return {k: v.astype(dtype) for k, v in got.items()}


@pytest.mark.parametrize("scale", [0.25, 64.0], ids=["ref<1", "ref>1"])
def test_check_grads_limit_is_tol_times_max_1_ref(scale):
    """(fp64 results, so that the injected error is the error; 0.25 and 64 are exact in binary)"""
    ref, tol = _ref(scale), 2.0 ** -10
    lim = tol * max(1.0, scale)
    errs = S.check_grads(_off(ref, "d_w", 0.99 * lim, np.float64), ref, tol=tol, scalar_term_tol=0.0, tag="under")
    assert errs["d_w"] == pytest.approx(0.99 * tol, rel=1e-9) and errs["d_zeta"] == 0.0
    with pytest.raises(AssertionError, match="d_w"):
        S.check_grads(_off(ref, "d_w", 1.01 * lim, np.float64), ref, tol=tol, scalar_term_tol=0.0, tag="over")
    if scale < 1:       # the limit is absolute below one: an error of tol * max|ref| is far inside it
        S.check_grads(_off(ref, "d_w", 3.9 * tol * scale, np.float64), ref, tol=tol, scalar_term_tol=0.0, tag="abs")


def test_check_grads_scalar_term_branch():
    ref, tol, stt = _ref(1.0), 2.0 ** -10, 2.0 ** -9          # limits: tol = 9.8e-4 plain, stt * 1e4 = 19.5 for the scalars
    err = 100.0 * tol
    for k in ("d_zeta", "d_nu"):
        S.check_grads(_off(ref, k, err), ref, tol=tol, scalar_term_tol=stt, tag="scalar")          # raised limit
        with pytest.raises(AssertionError, match=k):                                                # only when > 0
            S.check_grads(_off(ref, k, err), ref, tol=tol, scalar_term_tol=0.0, tag="off")
        with pytest.raises(AssertionError, match=k):                                                # never for fp64
            S.check_grads(_off(ref, k, err, np.float64), ref, tol=tol, scalar_term_tol=stt, tag="f64")
        with pytest.raises(AssertionError, match=k):                                                # torch fp64 neither
            S.check_grads({n: torch.from_numpy(v) for n, v in _off(ref, k, err, np.float64).items()}, ref, tol=tol,
                          scalar_term_tol=stt, tag="f64")
        with pytest.raises(AssertionError, match=k):                                                # the raised limit is one
            S.check_grads(_off(ref, k, 1.01 * stt * 1e4), ref, tol=tol, scalar_term_tol=stt, tag="beyond")
        bare = {n: v for n, v in ref.items() if not n.startswith("_")}                             # no sums: no branch
        with pytest.raises(AssertionError, match=k):
            S.check_grads(_off(ref, k, err), bare, tol=tol, scalar_term_tol=stt, tag="bare")
    with pytest.raises(AssertionError, match="d_w"):                                                # only the two scalars
        S.check_grads(_off(ref, "d_w", err), ref, tol=tol, scalar_term_tol=stt, tag="matrix")


def test_check_grads_fails_on_a_missing_key_and_ignores_diagnostics():
    ref = _ref(1.0)
    got = _off(ref, "d_w", 0.0)
    assert set(S.check_grads(got, ref, tol=1e-6, scalar_term_tol=0.0, tag="all")) == {"d_w", "d_zeta", "d_nu"}
    del got["d_nu"]
    with pytest.raises(AssertionError, match="d_nu.*missing"):
        S.check_grads(got, ref, tol=1e-6, scalar_term_tol=0.0, tag="missing")
    got = _off(ref, "d_w", 0.0)
    got["d_zeta"] = np.zeros((0,), np.float32)          # an output the operator left empty is absent too
    with pytest.raises(AssertionError, match="d_zeta.*missing"):
        S.check_grads(got, ref, tol=1e-6, scalar_term_tol=0.0, tag="empty")
    # _abs_* are not gradients: absent from got, of another shape, even NaN, they are not compared
    ref["_abs_zeta"], ref["_other"] = float("nan"), np.ones((7, 7))
    S.check_grads(_off(ref, "d_w", 0.0), ref, tol=1e-6, scalar_term_tol=0.0, tag="diagnostics")
    # and what got has beyond the reference is not looked at
    extra = _off(ref, "d_w", 0.0)
    extra["d_u"] = np.full((2, 2), np.nan, np.float32)
    S.check_grads(extra, ref, tol=1e-6, scalar_term_tol=0.0, tag="extra")


def test_check_grads_names_every_failing_entry_and_fails_on_nan():
    ref = _ref(1.0)
    got = _off(ref, "d_w", 1.0)
    got["d_nu"][0, 0] += 1.0
    with pytest.raises(AssertionError) as e:
        S.check_grads(got, ref, tol=1e-3, scalar_term_tol=0.0, tag="case-7")
    msg = str(e.value)
    assert "case-7" in msg and "d_w" in msg and "d_nu" in msg and "d_zeta" in msg      # (all relative errors are listed)
    assert msg.index("d_w") < msg.index("relative errors") and msg.index("d_nu") < msg.index("relative errors")
    bad = msg[:msg.index("relative errors")]
    assert "d_zeta" not in bad
    got = _off(ref, "d_w", 0.0)
    got["d_w"][1, 1] = np.nan
    with pytest.raises(AssertionError, match="d_w"):
        S.check_grads(got, ref, tol=1e-3, scalar_term_tol=0.0, tag="nan")


def test_check_grads_takes_the_operators_list_and_torch_tensors():
    ref = {k: np.arange(1.0, 5.0).reshape(2, 2) * (i + 1) for i, k in enumerate(S.GRAD_NAMES[:8])}
    e = torch.empty(0)
    outs = [torch.from_numpy(ref[k]).float() for k in S.GRAD_NAMES[:8]] + [e, e, e, e]
    assert set(S.check_grads(outs, ref, tol=1e-6, scalar_term_tol=0.0, tag="list")) == set(S.GRAD_NAMES[:8])
    outs[6] = outs[6].reshape(4)                        # compared in the reference's shape
    S.check_grads(outs, ref, tol=1e-6, scalar_term_tol=0.0, tag="flat")
    outs[7] = outs[7] + 1.0
    with pytest.raises(AssertionError, match="d_u"):
        S.check_grads(outs, ref, tol=1e-6, scalar_term_tol=0.0, tag="list")
    bf = [o.to(torch.bfloat16) for o in outs[:7]] + [outs[7].to(torch.bfloat16) - 1.0] + outs[8:]
    S.check_grads(bf, ref, tol=2.0 ** -8, scalar_term_tol=0.0, tag="bf16")


def test_there_is_no_default_tolerance():
    ref = _ref(1.0)
    for kw in (dict(scalar_term_tol=0.0, tag=""), dict(tol=1e-5, tag=""), dict(tol=1e-5, scalar_term_tol=0.0)):
        with pytest.raises(TypeError):
            S.check_grads(_off(ref, "d_w", 0.0), ref, **kw)
    assert S.SCALAR_TERM_TOL == 2e-7


# ---- the operator calls: fastgrnn_cuda.cpp:73-232, with recorders in place of the operators ---------------------------------

class _Recorder:
    def __init__(self, ret):
        self.calls, self.ret = [], ret

    def __call__(self, *a, **k):
        self.calls.append((a, k))
        return self.ret


@pytest.fixture
def ops(monkeypatch):
    hs, z, c = torch.zeros(1), torch.zeros(2), torch.zeros(3)
    fwd, bwd = _Recorder([hs, z, c]), _Recorder([torch.zeros(1)] * 12)
    monkeypatch.setattr(fastgrnn_cuda, "forward_unroll", fwd)
    monkeypatch.setattr(fastgrnn_cuda, "backward_unroll", bwd)
    return fwd, bwd


def _operands():
    P = {k: torch.full((1,), float(i)) for i, k in enumerate(("w", "u", "w1", "w2", "u1", "u2", "bias_gate",
                                                               "bias_update", "zeta", "nu"))}
    x, h0, G = torch.full((1,), 20.0), torch.full((1,), 21.0), torch.full((1,), 22.0)
    return P, x, h0, G


def _same_objects(got, want):
    return len(got) == len(want) and all(g is w for g, w in zip(got, want))


def test_forward_unroll_positional_list_and_keywords(ops):
    fwd, _ = ops
    P, x, h0, _ = _operands()
    S.forward_unroll(x, h0, P, "quantSigm")
    S.forward_unroll(x, h0, P, 1, update="quantTanh", flags=S.FLAG_SAVE_PREACT | S.FLAG_BATCH_MAJOR, want_gates=False)
    (a0, k0), (a1, k1) = fwd.calls
    # forward_unroll(input, w, u, bias_gate, bias_update, zeta, nu, initial_h, z_non_linearity, w1, w2, u1, u2)
    want = lambda gate: [x, P["w"], P["u"], P["bias_gate"], P["bias_update"], P["zeta"], P["nu"], h0, gate,
                         P["w1"], P["w2"], P["u1"], P["u2"]]
    assert _same_objects(a0[:8] + a0[9:], want(4)[:8] + want(4)[9:]) and a0[8] == 4, a0
    assert _same_objects(a1[:8] + a1[9:], want(1)[:8] + want(1)[9:]) and a1[8] == 1, a1
    assert k0 == dict(update_non_linearity=2, flags=0), k0
    assert k1 == dict(update_non_linearity=3, flags=20, want_gates=False), k1


def test_backward_unroll_positional_list_and_keywords(ops):
    _, bwd = ops
    P, x, h0, G = _operands()
    hs, z, aux = torch.zeros(1), torch.zeros(2), torch.zeros(3)
    S.backward_unroll(G, x, hs, z, aux, h0, P, "tanh")
    S.backward_unroll(G, x, hs, z, aux, h0, P, 0, update=3, flags=S.FLAG_SAVE_PREACT, bias_gate=P["bias_gate"],
                      bias_update=P["bias_update"], need_dx=False)
    (a0, k0), (a1, k1) = bwd.calls
    # backward_unroll(grad_h, input, hidden_states, zeta, nu, w, u, z, h_prime, initial_h, w1, w2, u1, u2, z_non_linearity)
    want = [G, x, hs, P["zeta"], P["nu"], P["w"], P["u"], z, aux, h0, P["w1"], P["w2"], P["u1"], P["u2"]]
    assert _same_objects(a0[:14], want) and a0[14] == 2 and len(a0) == 15, a0
    assert _same_objects(a1[:14], want) and a1[14] == 0 and len(a1) == 15, a1
    assert k0 == dict(update_non_linearity=2, flags=0), k0           # the biases are not passed unless named
    assert set(k1) == {"update_non_linearity", "flags", "bias_gate", "bias_update", "need_dx"}, k1
    assert k1["update_non_linearity"] == 3 and k1["flags"] == 4 and k1["need_dx"] is False
    assert k1["bias_gate"] is P["bias_gate"] and k1["bias_update"] is P["bias_update"]


def test_fwd_bwd_and_backward_of_pass_on_what_the_forward_saved(ops):
    fwd, bwd = ops
    P, x, h0, G = _operands()
    outs, grads = S.fwd_bwd(x, h0, G, P, "sigmoid", update="tanh", flags=S.FLAG_GRAD_LAST)
    assert outs is fwd.ret and grads is bwd.ret
    (fa, fk), (ba, bk) = fwd.calls[0], bwd.calls[0]
    assert fa[0] is x and fa[7] is h0 and fk == dict(update_non_linearity=2, flags=256)
    hs, z, c = fwd.ret
    assert _same_objects(ba[:3], [G, x, hs]) and ba[7] is z and ba[8] is c and ba[9] is h0 and ba[14] == 0
    assert bk == dict(update_non_linearity=2, flags=256), bk         # no biases, no need_dx: none were asked for
    # one saved tensor: given as z and as h_prime; the biases and need_dx go to the backward alone
    fwd.ret = [hs, z]
    S.fwd_bwd(x, h0, G, P, "relu", flags=S.FLAG_SAVE_PREACT, biases=True, need_dx=False)
    (fa, fk), (ba, bk) = fwd.calls[1], bwd.calls[1]
    assert fk == dict(update_non_linearity=2, flags=4) and fa[8] == 1
    assert ba[7] is z and ba[8] is z and ba[14] == 1
    assert set(bk) == {"update_non_linearity", "flags", "bias_gate", "bias_update", "need_dx"}
    assert bk["bias_gate"] is P["bias_gate"] and bk["bias_update"] is P["bias_update"] and bk["need_dx"] is False
    S.backward_of([hs, z, c], G, x, h0, P, "sigmoid", flags=S.FLAG_SAVE_PREACT, biases=True)
    ba, bk = bwd.calls[2]
    assert ba[7] is z and ba[8] is c and set(bk) == {"update_non_linearity", "flags", "bias_gate", "bias_update"}


def test_names_are_the_librarys():
    from kws_amd import _lib
    assert S.GRAD_NAMES == [n for n, _ in _lib.Grads._fields_]
    assert S.NONLINEARITY is _lib.NONLINEARITY and S.NONLINEARITY == O.GATE_CODES
    for name in dir(_lib):
        if name.startswith("FLAG_"):
            assert getattr(S, name) == getattr(_lib, name), name


# ---- the relu nudge --------------------------------------------------------------------------------------------------------

def test_relu_gates_end_up_off_the_kink():
    T, B, F, H, margin = 4, 3, 5, 8, 1e-2
    rng = np.random.default_rng(12)
    p = O.make_params(F, H, dtype=np.float32, seed=3, randomize_scalars=True)
    p["bias_gate"] = np.zeros_like(p["bias_gate"])                    # pre-activations on both sides of zero
    x = rng.standard_normal((T, B, F)).astype(np.float32)
    h0 = (0.5 * rng.standard_normal((B, H))).astype(np.float32)
    before = np.abs(S.relu_gate_preactivations(p, x, h0))
    assert before.shape == (T, B, H) and before.min() < margin        # (the case has something to move)
    kept = {k: v.copy() for k, v in p.items()}
    q = S.keep_relu_gates_off_the_kink(p, x, h0, margin=margin)
    assert all(np.array_equal(p[k], kept[k]) for k in p), "the caller's parameters were changed"
    assert np.abs(S.relu_gate_preactivations(q, x, h0)).min() >= margin
    moved = [k for k in p if not np.array_equal(p[k], q[k])]
    assert moved == ["bias_gate"] and q["bias_gate"].dtype == np.float32


# ---- the exact workspace -----------------------------------------------------------------------------------------------

class _HostExactWorkspace(S.ExactWorkspace):
    """the harness on host memory: the same buffer, cut so that the workspace slice is 256-byte aligned"""

    def _buffer(self, nbytes, dev):
        raw = torch.empty(nbytes + 2 * S.WS_MARGIN + 256, dtype=torch.uint8)
        big = raw[(-(raw.data_ptr() + S.WS_MARGIN)) % 256:][:nbytes + 2 * S.WS_MARGIN]
        big.fill_(0xA5)
        return big


def test_exact_workspace_hands_out_exact_slices_and_sees_writes_outside(monkeypatch):
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda dev=None: None)
    monkeypatch.setattr(fastgrnn_cuda, "_get_raw_stream", lambda idx: 77)
    monkeypatch.setattr(fastgrnn_cuda, "_ws_cache", {})
    import ctypes as C
    dev, cache, seen = torch.device("cpu"), fastgrnn_cuda._ws_cache, []

    def call(fn, what, tag, dev, nbytes, *args):
        ws = cache.get((None, 77))
        seen.append((what, nbytes, None if ws is None else (ws.numel(), ws.data_ptr() % 256, int(ws[0]))))
        if nbytes:
            base = ws.data_ptr()
            for off in fn(nbytes):              # fn: the byte offsets from the workspace's start that the "call" writes
                C.memset(base + off, 0, 1)

    exact = _HostExactWorkspace(call)
    exact(lambda n: [], "no workspace", "t", dev, 0)
    assert exact.checked == 0 and seen[-1] == ("no workspace", 0, None) and not cache
    exact(lambda n: [0, n - 1], "inside", "t", dev, 1000)
    assert exact.checked == 1 and seen[-1] == ("inside", 1000, (1000, 0, 0xA5)) and not cache
    with pytest.raises(AssertionError, match="past its 1000 workspace bytes"):
        exact(lambda n: [n], "one past", "t", dev, 1000)
    with pytest.raises(AssertionError, match="past its 1000 workspace bytes"):
        exact(lambda n: [n + S.WS_MARGIN - 1], "the margin's last byte", "t", dev, 1000)
    with pytest.raises(AssertionError, match="in front of its workspace"):
        exact(lambda n: [-1], "one in front", "t", dev, 1000)
    assert exact.checked == 1 and not cache                  # a failed call is not counted and the cache is put back
    held = cache[None, 77] = torch.zeros(8, dtype=torch.uint8)
    exact(lambda n: [5], "with a cached buffer", "t", dev, 256)
    assert cache[None, 77] is held and exact.checked == 2

    def grows(fn, what, tag, dev, nbytes, *args):            # a call that replaces the seeded slice is caught
        cache[None, 77] = torch.zeros(2 * nbytes, dtype=torch.uint8)
    with pytest.raises(AssertionError, match="took more"):
        _HostExactWorkspace(grows)(None, "took more", "t", dev, 256)
    assert cache[None, 77] is held
