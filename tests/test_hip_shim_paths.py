"""The Python operator shim's call paths on the GPU (kws_amd/fastgrnn_cuda.py): the validated-signature path against the
full checks bit for bit, the timing samples of every entry point, the refusals the two windowed forwards share, and the
flat parameter-gradient buffer.  Every case is T = 2, B = 17: one full tile and a ragged one, two workgroups, the
shortest sequence with a previous state.  Every call is valid or refused in Python before a launch."""
import pytest
import torch

from kws_amd import FastGRNNBatchNormCUDA, FastGRNNCUDA, _lib, fastgrnn_cuda as fc
from kws_amd.head import head_xent

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
T, B, R = 2, 17, 9


def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(DEV)


# ---- 1. the validated-signature path and the full checks give the same bits ----

# what the cached entries of a signature (fastgrnn_cuda._seen) carry, one predicate per cell shape of CELLS
def _plain(fwd, bwd):
    return fwd[3][2] is None and fwd[3][4] == 0 and not bwd[1]


def _optional_ws_and_dx(fwd, bwd):
    return fwd[0].forward_ws_optional and fwd[3][3] == 0 and bwd[2][4]      # no workspace asked for, d_x optional


def _rank_space(fwd, bwd):
    return fwd[3][2] == (T * B, fwd[0].rank_space_cols) and fwd[0].rank_space_cols > 0 and bwd[1]


def _zext_saved(fwd, bwd):
    return fwd[3][4] == fwd[0].zext.saved_bytes > 0 and bwd[0].zext.backward


CELLS = [pytest.param(128, 32, None, _plain, True, False, id="dense-H128-F32"),
         pytest.param(128, 64, None, _optional_ws_and_dx, True, False, id="dense-H128-F64"),
         pytest.param(256, 32, 8, _rank_space, True, False, id="lowrank-H256-F32-r8"),
         pytest.param(100, 24, None, _zext_saved, True, False, id="zero-extended-H100-F24"),
         pytest.param(128, 32, None, _plain, False, False, id="dense-H128-F32-no-dx"),
         pytest.param(128, 32, None, _plain, True, True, id="dense-H128-F32-last-state")]


@pytest.mark.parametrize("H,F,rank,carries,need_dx,last_state", CELLS)
def test_validated_path_equals_full_checks(monkeypatch, H, F, rank, carries, need_dx, last_state):
    torch.manual_seed(H + F)
    m = FastGRNNCUDA(F, H, wRank=rank, uRank=rank, device=DEV)
    x0, h0 = _randn(T, B, F, seed=1), 0.5 * _randn(B, H, seed=2)
    G = _randn(B, H, seed=3) if last_state else _randn(T, B, H, seed=3)
    full_checks = []
    describe = fc._describe
    monkeypatch.setattr(fc, "_describe", lambda *a: (full_checks.append(1), describe(*a))[1])

    def run():
        x, h = x0.clone().requires_grad_(need_dx), h0.clone().requires_grad_(True)
        for p in m.parameters():
            p.grad = None
        hs = m(x, h, last_state=last_state)
        hs.backward(G)
        torch.cuda.synchronize()
        return [hs.detach(), x.grad, h.grad] + [p.grad for p in m.parameters()]

    kept, use_seen = dict(fc._seen), fc._use_seen
    try:
        fc._seen.clear()
        fc._use_seen = False
        a = run()
        assert len(full_checks) == 2 and len(fc._seen) == 2
        fwd, = (v for k, v in fc._seen.items() if k[0] == "f")
        bwd, = (v for k, v in fc._seen.items() if k[0] == "b")
        assert carries(fwd, bwd), (fwd, bwd)
        assert bool(bwd[0].desc.flags & _lib.FLAG_NO_INPUT_GRAD) == (not need_dx)
        fc._seen.clear()
        fc._use_seen = True
        b = run()                                  # the first call of the signature: full checks, fills the entries
        assert len(full_checks) == 4 and len(fc._seen) == 2
        c = run()                                  # the validated-signature path
        assert len(full_checks) == 4 and len(fc._seen) == 2
    finally:
        fc._use_seen = use_seen
        fc._seen.update(kept)
    assert len(a) == 3 + len(list(m.parameters())) and a[0].shape == ((B, H) if last_state else (T, B, H))
    assert (a[1] is None) == (not need_dx)
    for i, (p, q, r) in enumerate(zip(a, b, c)):
        if p is None:
            assert q is None and r is None, i
        else:
            assert bool(torch.isfinite(p).all()) and torch.equal(p, q) and torch.equal(p, r), i


# ---- 2. one timing sample per call, under the tags bench.py and the tools filter on ----

def _cell(H, F):
    return dict(w=0.3 * _randn(H, F, seed=10), u=0.1 * _randn(H, H, seed=11), bg=_randn(1, H, seed=12),
                bu=_randn(1, H, seed=13), zeta=torch.full((1, 1), 0.7, device=DEV),
                nu=torch.full((1, 1), -2.5, device=DEV))


def _starts():
    return (torch.arange(B, dtype=torch.int32) % (R - T + 1)).to(DEV)          # 0 .. R - T, both ends included


def test_timing_tags():
    H, F = 128, 32
    P, e = _cell(H, F), torch.empty(0, device=DEV)
    x, h0, G = _randn(T, B, F, seed=1), 0.5 * _randn(B, H, seed=2), _randn(T, B, H, seed=3)
    pool, starts = _randn(R, F, seed=4), _starts()
    par = (P["w"], P["u"], P["bg"], P["bu"], P["zeta"], P["nu"])
    bn = FastGRNNBatchNormCUDA(F, H, device=DEV)
    assert bn._fused(x, False, B)
    labels = (torch.arange(B) % 12).to(DEV)
    fc._timing = samples = []
    try:
        hs, z, c = fc.forward_unroll(x, *par, h0, 0, e, e, e, e)
        fc.backward_unroll(G, x, hs, P["zeta"], P["nu"], P["w"], P["u"], z, c, h0, e, e, e, e, 0)
        fc.forward_unroll_affine(x, *par[:2], P["bg"].reshape(H), P["bu"].reshape(H), *par[4:],
                                 torch.ones(H, device=DEV), torch.ones(H, device=DEV), h0, 0)
        fc.forward_windows(pool, starts, T, *par, h0, 0)
        hw, saved = fc.forward_windows_train(pool, starts, T, *par, h0, 0)
        fc.backward_windows(G, pool, starts, T, hw, saved, P["zeta"], P["nu"], P["w"], P["u"], P["bg"], P["bu"], h0, 0)
        fc.frame_gemm(_randn(T * B, 64, seed=5), 0.3 * _randn(H, 64, seed=6))  # (the frame product starts at F = 64)
        assert [s[0] for s in samples] == ["forward", "backward", "forward_affine", "forward_windows",
                                           "forward_windows_train", "backward_windows", "frame_gemm"]
        # the calls that record no sample
        head_xent(hs[-1].contiguous(), 0.2 * _randn(12, H, seed=7), _randn(12, seed=8), labels)
        xb = x.clone().requires_grad_(True)
        bn(xb).backward(G)
        assert xb.grad is not None and len(samples) == 7
        torch.cuda.synchronize()
        for tag, e0, e1 in samples:
            assert e0.elapsed_time(e1) >= 0.0, tag
    finally:
        fc._timing = None


# ---- 3. the two windowed forwards refuse the same operands in the same words ----

def _bad_operands():
    H, F = 128, 32
    P = _cell(H, F)
    good = dict(pool=_randn(R, F, seed=4), starts=_starts(), h0=0.5 * _randn(B, H, seed=2), bg=P["bg"])
    over = _starts()
    over[3] = R - T + 1
    bad = {"3-D pool": dict(pool=good["pool"][None]),
           "float starts": dict(starts=_starts().float()),
           "initial_h [B+1,H]": dict(h0=_randn(B + 1, H, seed=2)),
           "bias_gate of H-1": dict(bg=P["bg"][:, :H - 1].contiguous()),
           "fp64 initial_h": dict(h0=good["h0"].double()),
           "start past the pool": dict(starts=over)}
    return P, good, bad


@pytest.mark.parametrize("which", ["3-D pool", "float starts", "initial_h [B+1,H]", "bias_gate of H-1", "fp64 initial_h",
                                   "start past the pool"])
def test_windowed_forwards_refuse_alike(which):
    P, good, bad = _bad_operands()
    a = dict(good, **bad[which])
    args = (a["pool"], a["starts"], T, P["w"], P["u"], a["bg"], P["bu"], P["zeta"], P["nu"], a["h0"], 0)
    raised = []
    for call in (fc.forward_windows, fc.forward_windows_train):
        with pytest.raises((RuntimeError, ValueError)) as e:
            call(*args)
        raised.append((type(e.value), str(e.value)))
    assert raised[0] == raised[1]
    assert raised[0][0] is (ValueError if which == "start past the pool" else RuntimeError)


# ---- 4. the parameter gradients of both backwards are views of one buffer ----

def test_parameter_gradients_share_one_buffer():
    H, F = 128, 32
    P, e = _cell(H, F), torch.empty(0, device=DEV)
    x, h0, G = _randn(T, B, F, seed=1), 0.5 * _randn(B, H, seed=2), _randn(T, B, H, seed=3)
    pool, starts = _randn(R, F, seed=4), _starts()
    par = (P["w"], P["u"], P["bg"], P["bu"], P["zeta"], P["nu"])
    hs, z, c = fc.forward_unroll(x, *par, h0, 0, e, e, e, e)
    g_unroll = fc.backward_unroll(G, x, hs, P["zeta"], P["nu"], P["w"], P["u"], z, c, h0, e, e, e, e, 0)
    hw, saved = fc.forward_windows_train(pool, starts, T, *par, h0, 0)
    g_windows = fc.backward_windows(G, pool, starts, T, hw, saved, P["zeta"], P["nu"], P["w"], P["u"], P["bg"], P["bu"],
                                    h0, 0)
    torch.cuda.synchronize()
    shapes = [(H, F), (H, H), (1, H), (1, H), (1, 1), (1, 1)]
    for g in (g_unroll, g_windows):
        assert len(g) == 12 and all(t.numel() == 0 for t in g[8:])
        views = [g[6], g[7], g[1], g[2], g[3], g[4]]           # registration order: W, U, bias_gate, bias_update, zeta, nu
        assert [tuple(v.shape) for v in views] == shapes
        assert len({v.untyped_storage().data_ptr() for v in views}) == 1
        offsets = [v.storage_offset() for v in views]
        assert offsets == [sum(a * b for a, b in shapes[:i]) for i in range(6)]
        assert views[0].untyped_storage().nbytes() == 4 * sum(a * b for a, b in shapes)
        assert all(bool(torch.isfinite(v).all()) for v in views)
