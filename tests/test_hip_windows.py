"""fastgrnn_hip_forward_windows on the GPU: utterances that are overlapping windows of a shared frame pool.

Shapes are the smallest that reach every address path: T = 7 frames, a pool of R = 61 rows, B = 37 windows (three
workgroups, the last one ragged; more than 32 utterances), and three sets of starts -- hop 1, hop 9 (disjoint windows
that leave pool rows unread) and a seeded permutation with repeats that includes 0 and R - T.

Every case checks, on one call of the C entry point into a caller-owned hs:
 1. the fp64 oracle on the materialised windows, under the bound the existing suites apply to hs of that shape:
    plain cells  max |hs - ref| / max(1, |ref|) <= 1e-5          (tests/test_hip_parity.py, tests/test_hip_stack.py)
    affine cells max |hs - ref| <= 4 e32 + 1e-5 max(1, max|ref|)  (tests/test_hip_batchnorm.py; e32: the same scan in
                                                                  fp32 torch ops against fp64)
 2. bit-equality with forward_unroll / forward_unroll_affine on the materialised [T,B,F] tensor (the variant changes
    addresses, not arithmetic; for F = 64 the frame GEMM's rows do not depend on their position)
 3. hs carries one extra trailing block of a sentinel and the pool a NaN tail: the sentinel is intact and no output is
    NaN (nothing written or read beyond the ragged batch or the pool).
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from kws_amd import FastGRNNCUDA, RNNClassifierModel, _lib, fastgrnn_cuda, fold_batchnorm
from kws_amd.rnn import gather_windows
from oracle import fastgrnn_oracle as O
from tests import batchnorm_golden as G
from tests import layer_cases as LC
from tests import support as S

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
A, BM, LAST = _lib.FLAG_PREACT_AFFINE, _lib.FLAG_BATCH_MAJOR, _lib.FLAG_HS_LAST
SHAPES = [(128, 32), (256, 32), (256, 64)]
T, R, B = 7, 61, 37
SENTINEL = -7777.0


@functools.lru_cache(maxsize=None)
def _pool(F):
    g = torch.Generator().manual_seed(1000 + F)
    return torch.randn(R, F, generator=g).to(DEV)


@functools.lru_cache(maxsize=None)
def _starts(kind):
    if kind == "hop1":
        s = torch.arange(B)
    elif kind == "hop9":                                   # 36 * 9 = 324 > R - T: the stream is 6 windows long, reused
        s = (torch.arange(B) % 7) * 9
        assert int(s.max()) == R - T
    else:
        g = torch.Generator().manual_seed(5)
        s = torch.randint(0, R - T + 1, (B,), generator=g)
        s[3], s[20], s[36] = 0, R - T, s[1]                # both ends and a repeat, the last one in the ragged tile
        s = s[torch.randperm(B, generator=g)]
    assert int(s.min()) == 0 and int(s.max()) <= R - T
    return s.to(torch.int32).to(DEV)


@functools.lru_cache(maxsize=None)
def _h0(H):
    g = torch.Generator().manual_seed(H)
    return (0.5 * torch.randn(B, H, generator=g)).to(DEV)


@functools.lru_cache(maxsize=None)
def _affine_cell(H, F, gate):
    m = G.random_bn(F, H, gate, seed=H + F + len(gate))
    return m, tuple(t.contiguous() for t in fold_batchnorm(m.cell))


@functools.lru_cache(maxsize=None)
def _reference(H, F, gate, affine, kind):
    """(materialised x [T,B,F], fp64 reference hs [T,B,H] on the device, bound as a callable on (hs, ref))."""
    x = gather_windows(_pool(F), _starts(kind), T).transpose(0, 1).contiguous()
    h0 = _h0(H)
    if affine:
        m, _ = _affine_cell(H, F, gate)
        ref = G.fp64_scan(m, x, h0)
        e32 = float((G.fp32_scan(m, x, h0).double() - ref).abs().max())
        bound = 4 * e32 + 1e-5 * max(1.0, float(ref.abs().max()))
        return x, ref, lambda hs: (float((hs.double() - ref).abs().max()), bound)
    p, _ = LC.plain_cell(H, F, gate)
    hs_o, _, _ = S.oracle64_forward(x.cpu().numpy(), p, h0.cpu().numpy(), gate)
    ref = torch.from_numpy(hs_o).to(DEV)
    return x, ref, lambda hs: (float(((hs.double() - ref).abs() / ref.abs().clamp(min=1.0)).max()), 1e-5)


def _operands(H, F, gate, affine):
    if affine:
        m, (w, u, bg, bu, sg, sc) = _affine_cell(H, F, gate)
        return w, u, bg, bu, m.cell.zeta, m.cell.nu, sg, sc
    _, P = LC.plain_cell(H, F, gate)
    return P["w"], P["u"], P["bias_gate"], P["bias_update"], P["zeta"], P["nu"], None, None


def _raw_windows(H, F, gate, flags, pool_buf, rows, starts, h0, hs_buf, ops):
    """One call of the C entry point into caller-owned buffers."""
    lib = _lib.load()
    w, u, bg, bu, zeta, nu, sg, sc = ops
    d = _lib.Desc(T, starts.numel(), F, H, 0, 0, S.NONLINEARITY[gate], 2, _lib.F32, flags)
    assert lib.fastgrnn_hip_windows_supported(C.byref(d)) == 1
    nbytes = int(lib.fastgrnn_hip_forward_windows_workspace_bytes(C.byref(d), rows))
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=DEV)
    ptr = lambda t: C.c_void_p(None if t is None else t.data_ptr())          # noqa: E731
    prm = _lib.Params(ptr(w), ptr(u), None, None, None, None, ptr(bg), ptr(bu), ptr(zeta), ptr(nu))
    st = lib.fastgrnn_hip_forward_windows(C.byref(d), C.byref(prm), ptr(sg), ptr(sc), ptr(pool_buf), rows, ptr(starts),
                                          ptr(h0), ptr(hs_buf), ptr(ws) if nbytes else None, nbytes,
                                          C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    assert st == 0, _lib.status_string(st)
    torch.cuda.synchronize()


def _existing_forward(H, F, gate, flags, x_tm, h0, ops):
    """forward_unroll / forward_unroll_affine on the materialised windows, in the layout of `flags`."""
    w, u, bg, bu, zeta, nu, sg, sc = ops
    x = x_tm.transpose(0, 1).contiguous() if flags & BM else x_tm
    if sg is not None:
        return fastgrnn_cuda.forward_unroll_affine(x, w, u, bg, bu, zeta, nu, sg, sc, h0, S.NONLINEARITY[gate],
                                                   flags=flags)
    return S.forward_unroll(x, h0, LC.plain_cell(H, F, gate)[1], gate, want_gates=False, flags=flags)[0]


@pytest.mark.parametrize("kind", ["hop1", "hop9", "perm"])
@pytest.mark.parametrize("layout", [0, BM, LAST], ids=["time_major", "batch_major", "last_state"])
@pytest.mark.parametrize("affine", [False, True], ids=["plain", "affine"])
@pytest.mark.parametrize("gate", ["sigmoid", "relu", "tanh"])
@pytest.mark.parametrize("H,F", SHAPES)
def test_windows_vs_oracle_existing_forward_and_sentinels(H, F, gate, affine, layout, kind):
    x_tm, ref, measure = _reference(H, F, gate, affine, kind)
    starts, h0 = _starts(kind), _h0(H)
    ops = _operands(H, F, gate, affine)
    flags = layout | (A if affine else 0)
    assert bool(torch.isfinite(ref).all())
    # the pool with a NaN tail of T rows behind it; hs with one more step / utterance / row block of the sentinel
    pool_buf = torch.cat([_pool(F), torch.full((T, F), float("nan"), device=DEV)])
    shape = (B + 1, H) if layout == LAST else ((B + 1, T, H) if layout == BM else (T + 1, B, H))
    hs_buf = torch.full(shape, SENTINEL, device=DEV)
    _raw_windows(H, F, gate, flags, pool_buf, R, starts, h0, hs_buf, ops)
    hs, tail = (hs_buf[:B], hs_buf[B:]) if layout else (hs_buf[:T], hs_buf[T:])
    assert bool((tail == SENTINEL).all()), "wrote beyond hs"
    assert not bool(torch.isnan(hs_buf).any()), "read beyond the pool"
    assert bool(torch.isnan(pool_buf[R:]).all()) and torch.equal(pool_buf[:R], _pool(F))
    # (1) the fp64 oracle (FLAG_HS_LAST: the bound is a property of the whole scan, the error that of its last step)
    if layout == LAST:
        got_tm = ref.clone()
        got_tm[-1] = hs.double()
    else:
        got_tm = hs.transpose(0, 1) if layout == BM else hs
    err, bound = measure(got_tm)
    print("H=%d F=%d %s %s layout=%d %s: error %.3g, bound %.3g" % (H, F, gate, "affine" if affine else "plain",
                                                                    layout, kind, err, bound))
    assert err <= bound
    # (2) the existing forward on the gathered windows: the same bits
    want = _existing_forward(H, F, gate, flags, x_tm, h0, ops)
    assert want.shape == hs.shape and torch.equal(want, hs)


def _plain_model(F):
    rng = np.random.default_rng(123)
    layers = [O.make_params(F, 256, dtype=np.float32, seed=41, randomize_scalars=True),
              O.make_params(256, 128, dtype=np.float32, seed=42, randomize_scalars=True)]
    fc_w = (0.2 * rng.standard_normal((12, 128))).astype(np.float32)
    fc_b = (0.1 * rng.standard_normal((12,))).astype(np.float32)
    m = RNNClassifierModel("FastGRNNCUDA", F, 2, [256, 128], [None, None], [None, None], [1.0, 1.0], [1.0, 1.0],
                           "sigmoid", "tanh", num_classes=12, device=DEV)
    with torch.no_grad():
        for rnn, p in zip(m.rnn_list, layers):
            S.copy_cell_params(rnn, p)
        m.hidden2keyword.weight.copy_(S.to_dev(fc_w)); m.hidden2keyword.bias.copy_(S.to_dev(fc_b))
    return m, layers, fc_w, fc_b


def _stream_windows(stream, hop, window):
    """[T, S*Nw, F]: the batch score_stream's windows make, gathered."""
    S, L, F = stream.shape
    nw = (L - window) // hop + 1
    starts = (torch.arange(S, device=DEV)[:, None] * L + torch.arange(nw, device=DEV)[None, :] * hop).reshape(-1)
    return gather_windows(stream.reshape(S * L, F), starts, window).transpose(0, 1).contiguous(), nw


@pytest.mark.parametrize("kind", ["FastGRNNCUDA", "FastGRNNBatchNorm", "FastGRNNBatchNormCUDA"])
def test_score_stream_equals_the_model_on_gathered_windows(kind):
    if kind == "FastGRNNCUDA":
        m, F = _plain_model(32)[0], 32
    else:
        _, full = G.trained_state_dict()
        m = RNNClassifierModel(kind, 64, 3, G.HIDDEN, [None] * 3, [None] * 3, [1.0] * 3, [1.0] * 3, "sigmoid", "tanh",
                               num_classes=G.CLASSES, device=DEV)
        m.load_state_dict(full, strict=True)
        m.eval()
        F = 64
    g = torch.Generator().manual_seed(9)
    stream = torch.randn(2, 23, F, generator=g).to(DEV)
    m.init_hidden()
    scores = m.score_stream(stream, hop=3, window=7)
    assert m.hidden_states == [None] * m.num_layers                        # neither read nor written
    assert scores.shape == (2, 6, 12) and not scores.requires_grad
    one = m.score_stream(stream[1], hop=3, window=7)                       # [L,F]: one stream
    assert one.shape == (1, 6, 12) and torch.equal(one[0], scores[1])
    x, nw = _stream_windows(stream, 3, 7)
    with torch.no_grad():
        m.init_hidden()
        want = m(x).reshape(2, nw, -1)
    m.init_hidden()
    err = float(((scores - want).abs() / want.abs().clamp(min=1.0)).max())
    print("%s score_stream vs model(windows): %.3g" % (kind, err))
    assert err <= 1e-5                                                     # (tests/test_hip_stack.py, scores)
    if kind == "FastGRNNCUDA":
        assert torch.equal(scores, want)
    if kind != "FastGRNNCUDA":
        m.train()
        with pytest.raises(NotImplementedError):
            m.score_stream(stream, hop=3, window=7)


def test_lowrank_cell_falls_back_to_gathered_windows():
    torch.manual_seed(3)
    m = FastGRNNCUDA(32, 256, wRank=8, uRank=8, device=DEV)
    assert not fastgrnn_cuda.windows_supported(T, B, 32, 256, w_rank=8, u_rank=8)
    pool, starts = _pool(32), _starts("perm")
    x = gather_windows(pool, starts, T).transpose(0, 1).contiguous()
    for last in (False, True):
        got = m.forward_windows(pool, starts, T, last_state=last)
        with torch.no_grad():
            want = m(x, last_state=last)
        assert not got.requires_grad and torch.equal(got, want)


def test_modules_take_int64_starts_and_batch_first():
    pool, starts = _pool(32), _starts("perm")
    m = FastGRNNCUDA(32, 128, device=DEV)
    a = m.forward_windows(pool, starts, T)
    b = m.forward_windows(pool, starts.long(), T)
    assert a.shape == (T, B, 128) and torch.equal(a, b) and not a.requires_grad
    m.batch_first = True
    c = m.forward_windows(pool, starts, T)
    assert c.shape == (B, T, 128) and torch.equal(c.transpose(0, 1), a)
    assert torch.equal(m.forward_windows(pool, starts, T, last_state=True), a[-1])
    bn, _ = _affine_cell(256, 64, "sigmoid")
    h = bn.forward_windows(_pool(64), starts, T, hiddenState=_h0(256))
    x = gather_windows(_pool(64), starts, T).transpose(0, 1).contiguous()
    with torch.no_grad():
        assert torch.equal(h, bn(x, _h0(256), training=False))


def test_range_check_is_on_the_host():
    """check=True: a start of R - T + 1 raises before anything is launched."""
    pool = _pool(32)
    m = FastGRNNCUDA(32, 128, device=DEV)
    bad = _starts("hop1").clone()
    bad[5] = R - T + 1
    with pytest.raises(ValueError):
        m.forward_windows(pool, bad, T)
    neg = _starts("hop1").clone().long()
    neg[0] = -1
    with pytest.raises(ValueError):
        m.forward_windows(pool, neg, T)
    with pytest.raises(ValueError):
        m.forward_windows(pool, _starts("hop1"), R + 1)
    P = LC.plain_cell(128, 32, "sigmoid")[1]
    with pytest.raises(ValueError):
        fastgrnn_cuda.forward_windows(pool, bad, T, P["w"], P["u"], P["bias_gate"], P["bias_update"], P["zeta"],
                                      P["nu"], _h0(128), 0)


def test_workload_geometry_against_the_oracle():
    """T = 99, hop 1, one stream of 99 + 255 frames (B = 256) through the default 64 -> 256 -> 128 model: the pool GEMM
    and the scans agree with the fp64 oracle of the stack beyond toy sizes (bound: tests/test_hip_stack.py, scores)."""
    m, layers, fc_w, fc_b = _plain_model(64)
    g = torch.Generator().manual_seed(17)
    stream = torch.randn(1, 99 + 255, 64, generator=g).to(DEV)
    scores = m.score_stream(stream, hop=1, window=99)
    assert scores.shape == (1, 256, 12)
    x, _ = _stream_windows(stream, 1, 99)
    l64 = [{k: v.astype(np.float64) for k, v in p.items()} for p in layers]
    _, scores_o, _, _, _, _, _ = O.stack_forward_backward(x.cpu().numpy().astype(np.float64), l64, fc_w.astype(np.float64),
                                                          fc_b.astype(np.float64), np.zeros(256, dtype=np.int64))
    err = (np.abs(scores[0].cpu().numpy() - scores_o) / np.maximum(1.0, np.abs(scores_o))).max()
    print("workload geometry: max rel error of the scores %.3g" % err)
    assert err <= 1e-5
