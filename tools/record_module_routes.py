#!/usr/bin/env python3
"""What the nn.Module classes hand to the operator shim, per case of tests/route_cases.py: every shim call in order (entry
point, shape / strides / dtype of its sequence argument, flags, want_gates, need_dx), the result's shape / strides /
dtype, and one sha256 over the result and every gradient.  The shim's entry points are wrapped by module attribute with
pass-through wrappers; nothing else of the package is touched, so the same file records any commit.

    python3 tools/record_module_routes.py OUT.json                 one recording (needs the GPU)
    python3 tools/record_module_routes.py --merge A.json B.json FIXTURE.json
                                                                   two recordings of one commit -> the fixture: a case
                                                                   whose digests differ keeps both and is named
"""
import hashlib
import inspect
import json
import os
import sys
import warnings
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import torch  # noqa: E402
import kws_amd  # noqa: E402
from kws_amd import batchnorm_train, fastgrnn_cuda  # noqa: E402
from tests import route_cases as RC  # noqa: E402

ENTRIES = ("forward_unroll", "backward_unroll", "forward_unroll_affine", "forward_windows", "forward_windows_train",
           "backward_windows")
LOGGED = ("flags", "want_gates", "need_dx", "batch_major", "last_state", "grad_last")
MAX_UNSTABLE = 3


def _meta(t):
    return [list(t.shape), list(t.stride()), str(t.dtype)]


class Recorder:
    """Context manager: the wrapped entry points append to ``self.calls`` while it is active."""

    def __enter__(self):
        self.calls, self._orig = [], {}
        for name in ENTRIES:
            self._orig[name] = fn = getattr(fastgrnn_cuda, name)
            setattr(fastgrnn_cuda, name, self._wrap(name, fn))
        self._call = batchnorm_train._call
        batchnorm_train._call = self._wrap_call(self._call)
        return self

    def __exit__(self, *exc):
        for name, fn in self._orig.items():
            setattr(fastgrnn_cuda, name, fn)
        batchnorm_train._call = self._call
        return False

    def _wrap(self, name, fn):
        sig = inspect.signature(fn)

        def wrapper(*a, **k):
            b = sig.bind(*a, **k)
            b.apply_defaults()
            args = b.arguments
            rec = {"entry": name, "seq": _meta(args["pool" if "pool" in args else "input"])}
            if "grad_h" in args:
                rec["grad_h"] = list(args["grad_h"].shape)
            rec.update({n: int(args[n]) for n in LOGGED if n in args})
            self.calls.append(rec)
            return fn(*a, **k)
        return wrapper

    def _wrap_call(self, fn):
        def wrapper(cfn, what, tag, dev, nbytes, desc, *rest):
            d = desc._obj
            self.calls.append({"entry": "batchnorm_train._call", "what": what,
                               "desc": [int(getattr(d, n)) for n, _ in type(d)._fields_]})
            return fn(cfn, what, tag, dev, nbytes, desc, *rest)
        return wrapper


def _seed_parameters(mod, gen):
    """Every parameter and running statistic from the seeded CPU generator, in name order."""
    with torch.no_grad():
        for name, t in sorted(list(mod.named_parameters()) + list(mod.named_buffers())):
            if not t.numel() or not t.is_floating_point():
                continue
            v = 0.1 * torch.randn(t.shape, generator=gen, dtype=torch.float64)
            if name.endswith("running_var"):
                v = 1.0 + v.abs()
            elif name.endswith(("bias_gate", "bias_update")) or (".bn_" in name and name.endswith("weight")):
                v = 1.0 + v
            t.copy_(v.to(t.dtype))


def _randn(gen, *shape):
    return torch.randn(*shape, generator=gen, dtype=torch.float32)


def _digest(tensors):
    h = hashlib.sha256()
    for t in tensors:
        if t is None:
            h.update(b"none")
        else:
            h.update(t.detach().cpu().reshape(-1).contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def _sequence(case, gen, dev, dtype, F):
    T, B = RC.T, RC.B
    layout = case["layout"]
    if layout == "btf":
        return _randn(gen, B, T, F).to(dtype).to(dev)
    if layout == "bft":
        return _randn(gen, B, F, T).to(dtype).to(dev).permute(2, 0, 1)
    if layout == "strided":
        return _randn(gen, T, B, F + 1).to(dtype).to(dev)[:, :, :F]
    x = _randn(gen, T, B, F).to(dtype)
    return x if layout == "cpu" else x.to(dev)


def _model_case(case, gen, dev):
    F, hidden, C = RC.MODEL
    dtype = getattr(torch, case["cell"])
    model = kws_amd.RNNClassifierModel("FastGRNNCUDA", F, len(hidden), hidden, [None] * 2, [None] * 2, [1.0] * 2, [1.0] * 2,
                                       "sigmoid", "tanh", num_classes=C, device=dev)
    _seed_parameters(model, gen)
    if case["method"] == "loss":
        x = _randn(gen, RC.T, RC.B, F).to(dtype).to(dev)
        labels = torch.randint(0, C, (RC.B,), generator=gen).to(dev)
        out = model.loss(x, labels)
        out.backward()
        return out, [p.grad for _, p in sorted(model.named_parameters())]
    stream = _randn(gen, 1, RC.STREAM_FRAMES, F).to(dtype).to(dev)
    return model.score_stream(stream, hop=1, window=RC.T), []


def run_case(case, dev):
    """-> {"calls": [...], "result": [shape, strides, dtype], "digest": hex}"""
    gen = torch.Generator().manual_seed(zlib.crc32(case["id"].encode()))
    with Recorder() as rec, warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        if case["cls"] == "RNNClassifierModel":
            out, grads = _model_case(case, gen, dev)
        else:
            out, grads = _module_case(case, gen, dev)
        torch.cuda.synchronize()
    return {"calls": rec.calls, "result": _meta(out), "digest": _digest([out] + grads)}


def _module_case(case, gen, dev):
    H, F, wRank, uRank, dtype, gate = RC.CELLS[case["cell"]]
    dtype = getattr(torch, dtype)
    mode, method = case["mode"], case["method"]
    bf = case["layout"] == "btf"
    cls = getattr(kws_amd, case["cls"])
    kw = dict(wRank=wRank, uRank=uRank) if case["cls"] == "FastGRNNCUDA" else {}
    mod = cls(F, H, gate_nonlinearity=gate, batch_first=bf, device=dev, **kw)
    if dtype == torch.float64:
        mod = mod.double()
    _seed_parameters(mod, gen)
    last = mode in ("grad_last", "nograd_last")
    call = dict(last_state=last)
    if "training" in case:
        call["training"] = case["training"]
    leaves = []
    if method == "forward":
        x = _sequence(case, gen, dev, dtype, F)
        if mode in ("grad_x", "grad_last"):
            x = x.detach().requires_grad_(True)
            leaves.append(x)
        if mode == "grad_x":
            pdt = torch.float32 if dtype == torch.bfloat16 else dtype
            h0 = (0.1 * _randn(gen, RC.B, H)).to(pdt).to(dev).requires_grad_(True)
            leaves.append(h0)
            call["hiddenState"] = h0
        fn, args = mod, (x,)
    else:
        pool = _randn(gen, RC.POOL_ROWS, F).to(dtype).to(dev)
        starts = torch.randint(0, RC.POOL_ROWS - RC.T + 1, (RC.B,), generator=gen, dtype=torch.int32).to(dev)
        fn, args = getattr(mod, method), (pool, starts, RC.T)
    if mode.startswith("grad"):
        out = fn(*args, **call)
        G = _randn(gen, *out.shape).to(out.dtype).to(dev)
        (out.float() * G.float()).sum().backward()
        grads = [t.grad for t in leaves] + [p.grad for _, p in sorted(mod.named_parameters())]
        return out, grads
    with (torch.inference_mode() if mode == "inference" else torch.no_grad()):
        return fn(*args, **call), []


def record(path):
    dev = torch.device("cuda:0")
    out = {}
    for case in RC.cases():
        out[case["id"]] = run_case(case, dev)
    with open(path, "w") as f:
        json.dump({"cases": out}, f, indent=0, sort_keys=True)
    print("recorded %d cases -> %s" % (len(out), path))


def merge(a_path, b_path, out_path):
    a, b = (json.load(open(p))["cases"] for p in (a_path, b_path))
    assert a.keys() == b.keys()
    unstable = sorted(k for k in a if a[k]["digest"] != b[k]["digest"])
    for k in a:
        ra, rb = dict(a[k]), dict(b[k])
        da, db = ra.pop("digest"), rb.pop("digest")
        assert ra == rb, "the route log of %s differs between the two recordings" % k
        if k in unstable:
            del a[k]["digest"]
            a[k]["digests"] = [da, db]
    if len(unstable) > MAX_UNSTABLE:          # a finding of its own: the route logs alone
        for r in a.values():
            r.pop("digest", None)
    with open(out_path, "w") as f:
        json.dump({"unstable": unstable, "cases": a}, f, indent=0, sort_keys=True)
    print("%d cases, %d with run-to-run different digests %s -> %s" % (len(a), len(unstable), unstable, out_path))


if __name__ == "__main__":
    if sys.argv[1] == "--merge":
        merge(*sys.argv[2:5])
    else:
        record(sys.argv[1])
