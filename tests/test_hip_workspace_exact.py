"""Every path-2 call, and the path-0 and path-1 calls listed below, stay inside a workspace of exactly the planned size
and do not depend on what lies in it.

Each case runs a forward and a backward through the Python operators twice: the ordinary way, and with every call's
workspace a 256-byte-aligned slice of exactly the bytes the call asks for, cut from a buffer filled with 0xA5 with
4 KiB on each side.  The margins must come back untouched and every output must equal the ordinary run's bit for bit.
A sha256 over every output of the case is compared with tests/golden/workspace_exact_digests.json, recorded on the GPU
from the library before its host code was reorganised (FASTGRNN_WS_DIGESTS_OUT=<file> records instead of comparing): the reorganised
launchers compute the same bits.  The path-0 (generic scan) and path-1 (fp32-MFMA scan) entries were recorded later, from
the build that first sized the generic backward's split-K partials by the largest product it forms: before it, the
three path-0 cases with a rank above H wrote 1 KiB, 128 bytes and 1 KiB past their workspace (inside the margins
here, with correct results).  The entries recorded first are unchanged."""
import hashlib
import json
import os

import pytest
import torch

from kws_amd import _lib, fastgrnn_cuda
from kws_amd import batchnorm_train
from tests import support as S

SP, BFT, ZE = _lib.FLAG_SAVE_PREACT, _lib.FLAG_X_BFT, _lib.FLAG_ZERO_EXTEND
GEN, F32M = _lib.FLAG_FORCE_GENERIC, _lib.FLAG_FORCE_F32_MFMA
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "workspace_exact_digests.json")
RECORD = os.environ.get("FASTGRNN_WS_DIGESTS_OUT")
# cases whose outputs differed between two recordings on the unchanged library: none
UNSTABLE = frozenset()
NONE = fastgrnn_cuda._NONE


def _rand(seed, dev):
    g = torch.Generator().manual_seed(seed)
    return lambda *shape, k=1.0, dtype=torch.float32: (k * torch.randn(*shape, generator=g)).to(dev).to(dtype)


def _cell(r, F, H, rw=0, ru=0):
    """w, u, bias_gate, bias_update, zeta, nu, w1, w2, u1, u2 in the operators' [out, in] layout"""
    w = NONE if rw else r(H, F, k=0.3)
    u = NONE if ru else r(H, H, k=0.08)
    w1, w2 = (r(rw, F, k=0.3), r(H, rw, k=0.3)) if rw else (NONE, NONE)
    u1, u2 = (r(ru, H, k=0.2), r(H, ru, k=0.2)) if ru else (NONE, NONE)
    return w, u, r(1, H, k=0.3), r(1, H, k=0.3), r(1, 1), r(1, 1), w1, w2, u1, u2


def _named(prefix, tensors):
    # (a FLAG_ZERO_EXTEND forward's saved tensor is an opaque uint8 buffer with padding nobody reads: not an output)
    return {"%s%d" % (prefix, i): t for i, t in enumerate(tensors) if t.numel() and t.dtype != torch.uint8}


def _unrolled(dev, F, H, T, B, flags, rw=0, ru=0, dtype=torch.float32):
    r = _rand(1000 * H + 10 * F + B + T, dev)
    P = dict(zip(("w", "u", "bias_gate", "bias_update", "zeta", "nu", "w1", "w2", "u1", "u2"), _cell(r, F, H, rw, ru)))
    x = r(*((B, F, T) if flags & BFT else (T, B, F)), dtype=dtype)
    h0, G = r(B, H, k=0.5), r(T, B, H, dtype=dtype)
    if dtype == torch.float64:                   # fp64 cells: every operand in fp64 (the same draws, widened)
        P, h0 = {k: v.double() for k, v in P.items()}, h0.double()
    fwd = S.forward_unroll(x, h0, P, "sigmoid", flags=flags)
    hs, z, h_prime = fwd[0], fwd[1], (fwd[2] if len(fwd) > 2 else NONE)      # (no third output: no h_prime is given)
    bwd = S.backward_unroll(G, x, hs, z, h_prime, h0, P, "sigmoid", flags=flags, bias_gate=P["bias_gate"],
                            bias_update=P["bias_update"])
    return {**_named("fwd", fwd), **_named("bwd", bwd)}


def _pool(dev, F, H, T, B):
    r = _rand(7000 + H + F + B, dev)
    cell = _cell(r, F, H)[:6]
    R = T + 3 * B
    starts = ((torch.arange(B) * 3) % (R - T + 1)).to(torch.int32).to(dev)     # overlapping windows
    return r, cell, r(R, F), starts, r(B, H, k=0.5)


def _windows(dev, F, H, T, B):
    r, (w, u, bg, bu, zeta, nu), pool, starts, h0 = _pool(dev, F, H, T, B)
    return {"hs": fastgrnn_cuda.forward_windows(pool, starts, T, w, u, bg, bu, zeta, nu, h0, 0)}


def _train_windows(dev, F, H, T, B):
    r, (w, u, bg, bu, zeta, nu), pool, starts, h0 = _pool(dev, F, H, T, B)
    hs, saved = fastgrnn_cuda.forward_windows_train(pool, starts, T, w, u, bg, bu, zeta, nu, h0, 0)
    bwd = fastgrnn_cuda.backward_windows(r(T, B, H), pool, starts, T, hs, saved, zeta, nu, w, u, bg, bu, h0, 0)
    return {"hs": hs, "saved": saved, **_named("bwd", bwd)}


def _batchnorm(dev, F, H, T, B):
    from kws_amd import FastGRNNBatchNormCUDA
    r = _rand(99, dev)
    torch.manual_seed(5)
    m = FastGRNNBatchNormCUDA(F, H, device=dev).train()
    with torch.no_grad():
        for p in m.parameters():
            p.add_(r(*p.shape, k=0.05))
    x = r(T, B, F).requires_grad_(True)
    hs = m(x, training=True)
    (hs * r(T, B, H)).sum().backward()
    out = {"hs": hs.detach(), "d_x": x.grad}
    out.update({"d_" + n: p.grad for n, p in m.named_parameters() if p.grad is not None})
    out.update({n: b for n, b in m.named_buffers() if b.is_floating_point()})
    return out


def _both(name, fn, **kw):
    """the case at B = 32 (two workgroups) and at the ragged B = 17"""
    return [("%s-B%d" % (name, B), fn, dict(kw, B=B)) for B in (32, 17)]


BF16 = torch.bfloat16
CASES_PATH_2 = (
    _both("h128_f32-sp-T3", _unrolled, F=32, H=128, T=3, flags=SP) +
    _both("h128_f64-sp", _unrolled, F=64, H=128, T=5, flags=SP) +
    _both("h128_f64-sp-bft", _unrolled, F=64, H=128, T=5, flags=SP | BFT) +
    _both("h256_f32", _unrolled, F=32, H=256, T=5, flags=0) +
    _both("h256_f32-bft", _unrolled, F=32, H=256, T=5, flags=BFT) +
    _both("h256_f64-bft", _unrolled, F=64, H=256, T=5, flags=BFT) +
    # the two shapes whose bf16 dU product once wrote past the workspace (head and body cut into chunks independently)
    [("h256_f32-bf16-sp-T50-B83", _unrolled, dict(F=32, H=256, T=50, B=83, flags=SP, dtype=BF16)),
     ("h256_f32-bf16-sp-T3-B1377", _unrolled, dict(F=32, H=256, T=3, B=1377, flags=SP, dtype=BF16))] +
    _both("lowrank-sp", _unrolled, F=32, H=256, T=5, flags=SP, rw=8, ru=8) +
    _both("lowrank-sp-bft", _unrolled, F=32, H=256, T=5, flags=SP | BFT, rw=8, ru=8) +
    _both("lowrank-bf16-sp", _unrolled, F=32, H=256, T=5, flags=SP, rw=8, ru=8, dtype=BF16) +
    _both("densified-h128-r8", _unrolled, F=32, H=128, T=5, flags=0, rw=8, ru=8) +
    _both("densified-h256-w17", _unrolled, F=32, H=256, T=5, flags=0, rw=17, ru=0) +
    _both("zext-h100_f20-sp", _unrolled, F=20, H=100, T=5, flags=SP | ZE) +
    _both("windows-h256_f64", _windows, F=64, H=256, T=5) +
    _both("train_windows-h128_f32", _train_windows, F=32, H=128, T=5) +
    _both("train_windows-h256_f64", _train_windows, F=64, H=256, T=5) +
    [("batchnorm-h128_f64-B6", _batchnorm, dict(F=64, H=128, T=3, B=6))]
)
# the generic scans: more than one trip of the unit loops; both ranks past the tiled GEMM's 64 columns, in fp64; a rank
# above H, where a factor's product is the largest the split-K partials hold (tests/generic_cases.py)
CASES_PATH_0 = [
    ("generic-h300_f20", _unrolled, dict(F=20, H=300, T=3, B=9, flags=GEN)),
    ("generic-h72_f80-r65-65-fp64", _unrolled, dict(F=80, H=72, T=3, B=9, flags=GEN, rw=65, ru=65, dtype=torch.float64)),
    ("generic-h8_f32-rw16", _unrolled, dict(F=32, H=8, T=3, B=5, flags=GEN, rw=16)),
    ("generic-h8_f13-ru20", _unrolled, dict(F=13, H=8, T=3, B=5, flags=GEN, ru=20)),
    ("generic-h8_f32-rw16-ru20", _unrolled, dict(F=32, H=8, T=3, B=5, flags=GEN, rw=16, ru=20)),
]
CASES_PATH_1 = [
    ("f32mfma-h128_f32-B48", _unrolled, dict(F=32, H=128, T=5, B=48, flags=F32M)),
    ("f32mfma-h64_f32-B37", _unrolled, dict(F=32, H=64, T=5, B=37, flags=F32M)),
    ("f32mfma-h128_f64-B16", _unrolled, dict(F=64, H=128, T=5, B=16, flags=F32M)),
]
CASES = CASES_PATH_2 + CASES_PATH_0 + CASES_PATH_1


def _assert_on_path(cases, path):
    for name, fn, kw in cases:
        if fn is _unrolled:
            k = dict(kw)
            dtype, flags = k.pop("dtype", torch.float32), k.pop("flags")
            rw, ru = k.pop("rw", 0), k.pop("ru", 0)
            for direction in (0, 1):
                assert fastgrnn_cuda.kernel_path(k["T"], k["B"], k["F"], k["H"], rw, ru, dtype=dtype, direction=direction,
                                                 flags=flags) == path, (name, direction)


def test_every_unrolled_case_is_on_kernel_path_2():
    _assert_on_path(CASES_PATH_2, 2)


def test_the_generic_and_f32_mfma_cases_are_on_paths_0_and_1():
    _assert_on_path(CASES_PATH_0, 0)
    _assert_on_path(CASES_PATH_1, 1)
    assert len(CASES_PATH_0) == 5 and len(CASES_PATH_1) == 3


def _digest(t):
    return hashlib.sha256(t.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


@pytest.mark.gpu
@pytest.mark.parametrize("name,fn,kw", CASES, ids=[c[0] for c in CASES])
def test_exact_workspace_untouched_margins_same_bits(monkeypatch, name, fn, kw):
    dev = torch.device("cuda:0")
    ordinary = fn(dev, **kw)
    torch.cuda.synchronize(dev)
    exact = S.ExactWorkspace(fastgrnn_cuda._call)
    monkeypatch.setattr(fastgrnn_cuda, "_call", exact)
    monkeypatch.setattr(batchnorm_train, "_call", exact)
    again = fn(dev, **kw)
    torch.cuda.synchronize(dev)
    assert exact.checked >= 1, "no call of the case took a workspace"
    assert ordinary.keys() == again.keys() and len(ordinary) >= 1
    for k in ordinary:
        assert ordinary[k].dtype == again[k].dtype and ordinary[k].shape == again[k].shape, (name, k)
        assert torch.equal(ordinary[k].contiguous().view(torch.uint8), again[k].contiguous().view(torch.uint8)), (name, k)
    # one digest per case over every output: sha256 of the lines "<output>=<sha256 of its bytes>" sorted by output name
    per_output = "".join("%s=%s\n" % (k, _digest(again[k])) for k in sorted(again))
    digest = hashlib.sha256(per_output.encode()).hexdigest()
    if RECORD:
        table = json.load(open(RECORD)) if os.path.exists(RECORD) else {}
        table[name] = digest
        with open(RECORD, "w") as f:
            json.dump(table, f, indent=0, sort_keys=True)
    elif name not in UNSTABLE:
        assert json.load(open(GOLDEN))[name] == digest, (name, per_output)
