"""The module-level route cases (tests/golden/routes/parent.json): calls of the nn.Module classes at the smallest sizes
at which a layout / flag / saved-tensor decision can still differ -- T = 2 (the shortest sequence with a previous step),
B = 17 (one full 16-row tile and a ragged one: two workgroups; no size-1 dimension, so a permuted view is really
non-contiguous).  Shared by tools/record_module_routes.py, which recorded what the modules hand to the operator shim
before their routing was gathered into ``kws_amd._route``, tests/test_hip_module_routes.py, which replays the table on
the GPU, and tests/test_module_routes_cpu.py, which derives the recorded calls from the route record alone."""
T, B = 2, 17
POOL_ROWS = 40                  # frames in the pool of a windowed case
STREAM_FRAMES = 18              # score_stream: window T, hop 1 -> B windows of one stream
MODEL = (32, [256, 128], 12)    # RNNClassifierModel: input, hidden sizes, classes

# name -> (H, F, wRank, uRank, dtype, gate)
CELLS = {
    "h128f32": (128, 32, None, None, "float32", "sigmoid"),
    "h128f64": (128, 64, None, None, "float32", "sigmoid"),
    "h256f32": (256, 32, None, None, "float32", "sigmoid"),
    "h256f64": (256, 64, None, None, "float32", "sigmoid"),
    "h256f32_r8r8": (256, 32, 8, 8, "float32", "sigmoid"),
    "h256f32_w8": (256, 32, 8, None, "float32", "sigmoid"),
    "h100f24": (100, 24, None, None, "float32", "sigmoid"),          # zero-extended
    "h300f32": (300, 32, None, None, "float32", "sigmoid"),          # kernel path 0
    "h128f32_fp64": (128, 32, None, None, "float64", "sigmoid"),
    "h128f32_bf16": (128, 32, None, None, "bfloat16", "sigmoid"),
    "h256f64_bf16": (256, 64, None, None, "bfloat16", "sigmoid"),
    "h128f32_relu": (128, 32, None, None, "float32", "relu"),
    "h128f32_tanh": (128, 32, None, None, "float32", "tanh"),
}
GATE_VARIANTS = ("h128f32_relu", "h128f32_tanh")
DENSE = ("h128f32", "h128f64", "h256f32", "h256f64", "h100f24", "h300f32", "h128f32_fp64")   # what the BatchNorm cell takes

# layouts of x: contiguous [T,B,F]; [B,T,F] on a batch_first module; permute(2,0,1) of the loader's [B,F,T]; a strided
# view that is no such view (the first F columns of a [T,B,F+1] tensor); a CPU tensor (moved by the module)
LAYOUTS = ("tbf", "btf", "bft", "strided")
# grad_x: autograd, full hs, x and an explicit h0 require grad; grad: autograd, full hs, x does not, default h0;
# grad_last: autograd with last_state (x requires grad); the rest run no backward
MODES = ("grad_x", "grad", "grad_last", "nograd", "nograd_last", "inference")


def _case(cls, cell, layout, mode, method="forward", **extra):
    d = dict(cls=cls, cell=cell, layout=layout, mode=mode, method=method, **extra)
    d["id"] = "-".join([cls, method, cell, layout, mode] + ["%s=%s" % kv for kv in sorted(extra.items())])
    return d


def cases():
    out = []
    for cell in CELLS:
        if cell in GATE_VARIANTS:
            out += [_case("FastGRNNCUDA", cell, "tbf", m) for m in MODES]
            continue
        for layout in LAYOUTS:
            modes = ("grad_x", "nograd") if layout == "strided" else MODES
            out += [_case("FastGRNNCUDA", cell, layout, m) for m in modes]
    out += [_case("FastGRNNCUDA", "h128f32", "cpu", m) for m in ("grad", "nograd")]
    for cell in DENSE:
        for layout in LAYOUTS:
            out += [_case("FastGRNNBatchNorm", cell, layout, m, training=False) for m in ("nograd", "nograd_last")]
    for cell in ("h128f64", "h300f32"):
        for layout in ("tbf", "btf"):
            out += [_case("FastGRNNBatchNormCUDA", cell, layout, m, training=False) for m in ("nograd", "nograd_last")]
    for cell in ("h128f32", "h256f64", "h300f32"):       # (the last one: the per-frame torch formula)
        for layout in ("tbf", "btf"):
            out += [_case("FastGRNNBatchNormCUDA", cell, layout, m, training=True) for m in ("grad_x", "grad_last")]
    for cell in ("h128f32", "h256f64", "h256f32_r8r8", "h128f32_bf16"):    # two supported, two gathered
        for method, modes in (("forward_windows", ("nograd", "nograd_last")), ("unroll_windows", ("grad", "grad_last"))):
            out += [_case("FastGRNNCUDA", cell, "pool", m, method) for m in modes]
    for cell in ("h128f32", "h300f32"):
        out += [_case("FastGRNNBatchNorm", cell, "pool", m, "forward_windows", training=False)
                for m in ("nograd", "nograd_last")]
    for dtype in ("float32", "bfloat16"):
        out += [_case("RNNClassifierModel", dtype, "tbf", "grad", "loss"),
                _case("RNNClassifierModel", dtype, "stream", "nograd", "score_stream")]
    assert len({c["id"] for c in out}) == len(out)
    return out


def input_meta(case):
    """(shape, strides) of the sequence the module is called with, as the layout defines them."""
    F = CELLS[case["cell"]][1]
    return {"tbf": ((T, B, F), (B * F, F, 1)), "cpu": ((T, B, F), (B * F, F, 1)), "btf": ((B, T, F), (T * F, F, 1)),
            "bft": ((T, B, F), (1, F * T, T)), "strided": ((T, B, F), (B * (F + 1), F + 1, 1))}[case["layout"]]
