"""GPU tests of the work partitions between the suite's small shapes and B = 4096: the frame / d_x GEMM
(rows_gemm_split), the weight-gradient GEMMs (tn_gemm_big, tn_gemm_w4, tn_big_reduce) and the slab reductions at the
(T, B) shapes of tests/partition_cases.py -- chunks of 1 to 5 stages with short and full last chunks, partial last
stages inside multi-stage chunks, idle and padded workgroups, both dU routes, the bf16 head / body split, and slab
reductions of 128, 129, 130 and 257 workgroups.

Every comparison is against the fp64 oracle (oracle/fastgrnn_oracle.py) or an fp64 product under the bounds the suite
already holds these kernels to at full size, or exact (bit for bit) where the kernels promise it.  The helpers are those
of tests/support.py; the cases shared with test_hip_stack.py, test_hip_bft_wide.py, test_hip_parity.py and
test_hip_bn_train.py are in tests/layer_cases.py and tests/bn_train_golden.py.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import fastgrnn_oracle as O
from tests import bn_train_golden as BN
from tests import layer_cases as LC
from tests import partition_cases as PC
from tests import support as S
from tests.support import DEV

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from kws_amd import _lib, fastgrnn_cuda

LAYERS = [(256, 32), (256, 64), (256, 128), (128, 64), (128, 128), (128, 256)]        # (H, F): GEMMs around the scan
FRAME = [(128, 64), (128, 128), (128, 256), (256, 64), (256, 128)]                   # (H, F) of fastgrnn_hip_frame_gemm
# below, at and above one stage; 256 stages (one each) and 257 / 258 / 514 (chunks of 2 and 3, tails 1, 1 and 29);
# 770 stages (chunks of 4, last of 2, tail 25) and 1026 (chunks of 5, last of 1)
FRAME_ROWS = [1, 31, 32, 33, 8192, 8193, 8225, 16445, 24633, 32823]
ODD_T, EVEN_B = (5, 3289), (5, 2080)      # multi-stage chunks with odd T and a tail / with B a multiple of 32
_ids = lambda v: "x".join(str(i) for i in v) if isinstance(v, tuple) else str(v)  # noqa: E731


def test_frame_rows_are_what_the_comment_says():
    cuts = [PC.rows_gemm_cut(R) for R in FRAME_ROWS]
    assert [c.spw for c in cuts] == [1, 1, 1, 1, 1, 2, 2, 3, 4, 5]
    assert [c.last for c in cuts[5:]] == [1, 2, 1, 2, 1] and FRAME_ROWS[-1] == max(FRAME_ROWS)


# ---- (a) the frame GEMM by itself ------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("H,F", FRAME, ids=_ids)
def test_frame_gemm_rows_do_not_depend_on_the_cut(H, F, bf16):
    """fastgrnn_hip_frame_gemm through the C ABI into a buffer 64 rows too long, filled with NaN: rows >= R stay NaN;
    row r of the product over the first R rows has the bits of row r of the product over all 32 823, for every R of
    FRAME_ROWS (a row's sum does not depend on its place in a stage or chunk); the longest product against fp64 (for
    bf16 x on the rounded values), elementwise relative to max(1, |ref|), at most four times what numpy's fp32 product
    loses on the same operands (the margin of test_hip_fuzz.py).

    Measured on an MI355X over the ten (H, F, type) cases: the kernel loses 3.0e-7 (H=128, F=64) to 9.2e-7 (H=128,
    F=256, bf16), numpy's fp32 product 9.1e-7 to 3.7e-6 on the same operands; the ratio is 0.24 to 0.38, bound 4."""
    lib = _lib.load()
    rng = np.random.default_rng(4000 + H + F)
    Rmax = FRAME_ROWS[-1]
    w = O.make_params(F, H, dtype=np.float32, seed=51)["w"]
    xt = torch.from_numpy(rng.standard_normal((Rmax, F)).astype(np.float32)).to(DEV)
    if bf16:
        xt = xt.to(torch.bfloat16)
    wt = S.to_dev(w)
    dtype = _lib.BF16_IO if bf16 else _lib.F32

    def product(R):
        out = torch.full((R + 64, H), float("nan"), dtype=torch.float32, device=DEV)
        torch.cuda.synchronize()
        st = lib.fastgrnn_hip_frame_gemm(R, H, F, C.c_void_p(xt.data_ptr()), C.c_void_p(wt.data_ptr()),
                                         C.c_void_p(out.data_ptr()), dtype, C.c_void_p(None))
        assert st == 0, (R, _lib.status_string(st))
        torch.cuda.synchronize()
        assert bool(torch.isnan(out[R:]).all()), "rows beyond R = %d were written" % R
        assert not bool(torch.isnan(out[:R]).any()), "rows below R = %d were left out" % R
        return out[:R]

    full = product(Rmax)
    for R in FRAME_ROWS[:-1]:
        part = product(R)
        same = (part.view(torch.int32) == full[:R].view(torch.int32)).all(dim=1)
        assert bool(same.all()), (R, "first differing row", int((~same).nonzero()[0]))
    x_used = xt.float().cpu().numpy()
    ref64 = x_used.astype(np.float64) @ w.astype(np.float64).T
    den = np.maximum(1.0, np.abs(ref64))
    e_k = float((np.abs(full.cpu().numpy().astype(np.float64) - ref64) / den).max())
    e_32 = float((np.abs((x_used @ w.T).astype(np.float64) - ref64) / den).max())
    print("frame_gemm H=%d F=%d %s: kernel %.3e numpy-fp32 %.3e ratio %.2f" % (H, F, "bf16" if bf16 else "f32", e_k, e_32,
                                                                               e_k / e_32))
    assert e_k <= 4.0 * e_32, (e_k, e_32)


# ---- (b) whole layers against the fp64 oracle --------------------------------------------------------------------
def _draw(T, B, F, H):
    """inputs as test_hip_stack.test_stack_layer_shapes_on_the_matrix_pipe_vs_oracle draws them"""
    rng = np.random.default_rng(1000 + T * 7 + B + F)
    p = O.make_params(F, H, dtype=np.float32, seed=31, randomize_scalars=True)
    x = rng.standard_normal((T, B, F)).astype(np.float32)
    h0 = (0.5 * rng.standard_normal((B, H))).astype(np.float32)
    G = rng.standard_normal((T, B, H)).astype(np.float32)
    return p, x, h0, G


def _scalar_tol(H, F):
    # d_zeta / d_nu are also bounded by SCALAR_TERM_TOL of the sum of their terms' magnitudes, on every shape: at
    # (H, F, T, B) = (256, 32, 99, 83) d_zeta = 18.1 is what is left of terms that sum to 1.6e5 in magnitude; the kernel
    # is 2.8e-5 of the result off (3e-9 of the terms), the oracle evaluated in fp32 3.3e-5 -- neither meets a plain 2e-5
    return S.SCALAR_TERM_TOL


def _scalar_ratio(gr, g_o, H, F):
    """error of d_zeta / d_nu over the bound S.check_grads holds them to (reporting only)"""
    worst = 0.0
    for k, n in ((3, "zeta"), (4, "nu")):
        ref = float(np.asarray(g_o["d_" + n]).ravel()[0])
        lim = max(2e-5 * max(1.0, abs(ref)), _scalar_tol(H, F) * g_o["_abs_" + n])
        worst = max(worst, abs(float(gr[k].reshape(-1)[0]) - ref) / lim)
    return worst


def _assert_path_2(T, B, F, H, flags, **kw):
    for direction in (0, 1):
        assert fastgrnn_cuda.kernel_path(T, B, F, H, direction=direction, flags=flags, **kw) == 2, (T, B, F, H, direction)


@pytest.mark.parametrize("T,B", PC.SHAPES, ids=_ids)
@pytest.mark.parametrize("H,F", LAYERS, ids=_ids)
def test_layer_forward_and_backward_vs_oracle(H, F, T, B):
    """hs and the saved pre-activation to 1e-5, all eight gradients to 2e-5 of max(1, max|ref|) (d_zeta / d_nu with
    SCALAR_TERM_TOL of their terms' magnitudes as well, see _scalar_tol).  Measured on an MI355X over the 114 cases: hs
    7.1e-6 and the pre-activation 7.1e-6 at worst (0.71 of the bound, H=256 / F=32 at T=99, B=83); d_x, d_h0, d_w, d_u
    and the bias gradients 1.2e-6 at worst (0.06 of the bound); d_zeta / d_nu up to 2.3e-4 of the result on the wide
    H=256 layers at (7, 3519), where the result is a small remainder of its terms: 0.07 of their bound at worst (the
    ratio is printed).  Against the plain 2e-5 of the result alone d_zeta of H=256 / F=32 at (99, 83) is at 1.38."""
    _assert_path_2(T, B, F, H, _lib.FLAG_SAVE_PREACT)
    p, x, h0, G = _draw(T, B, F, H)
    outs, gr = LC.layer_fwd_bwd(S.to_dev(x), S.to_dev(h0), S.to_dev(G), p, preact=True)
    hs_o, zs_o, cs_o, g_o = S.oracle64(x, G, p, h0)
    e_hs = float(np.abs(outs[0].cpu().numpy() - hs_o).max())
    e_pre = float(np.abs(outs[1].cpu().numpy() - S.dense_preactivation64(x, p, h0, hs_o)).max())
    print("layer H=%d F=%d T=%d B=%d: hs %.2e pre %.2e (of 1e-5)" % (H, F, T, B, e_hs, e_pre))
    assert e_hs <= 1e-5 and e_pre <= 1e-5, (e_hs, e_pre)
    errs = S.check_grads(gr, g_o, tol=2e-5, scalar_term_tol=_scalar_tol(H, F), tag=(H, F, T, B))
    print("layer H=%d F=%d T=%d B=%d: worst gradient %.2e (of 2e-5) %s; scalars / their bound %.2f"
          % (H, F, T, B, max(errs.values()), {k: "%.1e" % v for k, v in errs.items()}, _scalar_ratio(gr, g_o, H, F)))


@pytest.mark.parametrize("T,B", [(3, 2731), ODD_T, EVEN_B], ids=_ids)
def test_layer_reference_contract_vs_oracle(T, B):
    """the reference operator's own saved pair (z_s, h_prime_s) instead of the pre-activation, H=256 / F=64"""
    H, F = 256, 64
    _assert_path_2(T, B, F, H, 0)
    p, x, h0, G = _draw(T, B, F, H)
    outs, gr = LC.layer_fwd_bwd(S.to_dev(x), S.to_dev(h0), S.to_dev(G), p, preact=False)
    hs_o, zs_o, cs_o, g_o = S.oracle64(x, G, p, h0)
    assert np.abs(outs[0].cpu().numpy() - hs_o).max() <= 1e-5
    assert np.abs(outs[1].cpu().numpy() - zs_o).max() <= 1e-5 and np.abs(outs[2].cpu().numpy() - cs_o).max() <= 1e-5
    S.check_grads(gr, g_o, tol=2e-5, scalar_term_tol=_scalar_tol(H, F), tag=(T, B))


# ---- (c) a sparse gradient on the seam rows ----------------------------------------------------------------------
@pytest.mark.parametrize("T,B", PC.SHAPES, ids=_ids)
@pytest.mark.parametrize("H,F", LAYERS, ids=_ids)
def test_gradient_of_the_seam_utterances_alone(H, F, T, B):
    """grad_hs is zero but for b = 0, b = B - 1 and the utterances whose rows sit on either side of a chunk boundary
    (partition_cases.seam_utterances): d_x and d_h0 of every other utterance are exactly zero, and the parameter
    gradients are those of the oracle run on these B' utterances alone -- a row counted twice or not at all is 1 / B'
    of such a sum, not 1 / R."""
    bs = PC.seam_utterances(T, B)
    p, x, h0, _ = _draw(T, B, F, H)
    G = np.zeros((T, B, H), np.float32)
    G[:, bs] = np.random.default_rng(7 + B).standard_normal((T, len(bs), H)).astype(np.float32)
    outs, gr = LC.layer_fwd_bwd(S.to_dev(x), S.to_dev(h0), S.to_dev(G), p, preact=True)
    rest = torch.ones(B, dtype=torch.bool, device=DEV)
    rest[bs] = False
    assert int((gr[0][:, rest] != 0).sum()) == 0 and int((gr[5][rest] != 0).sum()) == 0
    _, _, _, g_o = S.oracle64(np.ascontiguousarray(x[:, bs]), np.ascontiguousarray(G[:, bs]), p, np.ascontiguousarray(h0[bs]))
    errs = S.check_grads([gr[0][:, bs], gr[1], gr[2], gr[3], gr[4], gr[5][bs], gr[6], gr[7]], g_o, tol=2e-5,
                         scalar_term_tol=_scalar_tol(H, F), tag=(H, F, T, B))
    print("seams H=%d F=%d T=%d B=%d (%d utterances): worst gradient %.2e (of 2e-5)" % (H, F, T, B, len(bs),
                                                                                      max(errs.values())))


# ---- (d) layouts and types that take other branches ----------------------------------------------------------------
@pytest.mark.parametrize("T,B", [ODD_T, EVEN_B], ids=_ids)
@pytest.mark.parametrize("H,F", [(256, 64), (128, 256)], ids=_ids)
def test_bft_frames_bitwise_equal_to_the_time_major_call(H, F, T, B):
    """FASTGRNN_FLAG_X_BFT (rows_gemm_split<BFT_IN> enumerates rows utterance-major; the backward runs on a time-major
    workspace copy): the same bits as the time-major call, forward and backward"""
    SP, BFT = _lib.FLAG_SAVE_PREACT, _lib.FLAG_X_BFT
    _assert_path_2(T, B, F, H, SP | BFT)
    x, xb, h0, G = LC.bft_data(T, B, F, H)
    P = LC.bft_params(F, H, seed=11 + B % 7)
    o_tm, o_bft = S.forward_unroll(x, h0, P, "sigmoid", flags=SP), S.forward_unroll(xb, h0, P, "sigmoid", flags=SP | BFT)
    S.assert_same_bits(o_bft[0], o_tm[0], "preact hs"); S.assert_same_bits(o_bft[1], o_tm[1], "preact z")
    LC.compare_bft_backward(G, x, xb, o_tm, o_bft, h0, P, "sigmoid", SP, "preact")


@pytest.mark.parametrize("T,B", [ODD_T, EVEN_B], ids=_ids)
def test_batch_major_takes_the_periodic_dU_gemm(T, B):
    """FASTGRNN_FLAG_BATCH_MAJOR on H=256 / F=32 (tn_gemm_big_run_periodic): bit-equal to the time-major call wherever
    test_stack_layer_batch_major_and_last_state_contracts asserts it -- hs, the pre-activation, d_x and every gradient
    whose sum does not follow the rows' memory order -- and d_w / d_u, which do, against the oracle"""
    H, F = 256, 32
    BM = _lib.FLAG_BATCH_MAJOR
    _assert_path_2(T, B, F, H, _lib.FLAG_SAVE_PREACT | BM)
    p, x, h0, G = _draw(T, B, F, H)
    xt, ht, Gt = S.to_dev(x), S.to_dev(h0), S.to_dev(G)
    outs, gr = LC.layer_fwd_bwd(xt, ht, Gt, p, preact=True)
    outs_b, gr_b = LC.layer_fwd_bwd(xt.transpose(0, 1).contiguous(), ht, Gt.transpose(0, 1).contiguous(), p, flags=BM, preact=True)
    assert torch.equal(outs_b[0].transpose(0, 1), outs[0]) and torch.equal(outs_b[1].transpose(0, 1), outs[1])
    assert torch.equal(gr_b[0].transpose(0, 1), gr[0])
    for k in (1, 2, 3, 4, 5):
        assert torch.equal(gr[k], gr_b[k]), S.GRAD_NAMES[k]
    _, _, _, g_o = S.oracle64(x, G, p, h0)
    S.check_grads([gr_b[0].transpose(0, 1)] + list(gr_b[1:8]), g_o, tol=2e-5, scalar_term_tol=_scalar_tol(H, F),
                  tag=(T, B))


@pytest.mark.parametrize("T,B", [(11, 1499), EVEN_B, (3, 1377)], ids=_ids)
@pytest.mark.parametrize("H,F", [(256, 32), (128, 256)], ids=_ids)
def test_bf16_sequences_where_head_and_body_are_cut_differently(H, F, T, B):
    """bf16 sequences: on H=256 dU is an fp32 head over the B rows of h0 and a bf16 body over the rest, cut into chunks
    independently ((11, 1499): 47 one-stage chunks and 118 of 4 stages; (5, 2080): 65 and 87 of 3); at (3, 1377) they
    make 44 + 87 partials, one more than twice the 65 of the whole product, which the workspace once had no room for
    (tests/test_partition_cases_cpu.py).  Reference and bounds of test_bf16_sequences_fp32_master_grads."""
    if H == 256:
        body, head = PC.tn_partials(T * B, 2, shift=B, bf16=True)
        assert head > 0 and body != head, (body, head)
        if (T, B) == (3, 1377):
            assert body + head == PC.tn_slots(T * B, 2) + 1
    LC.bf16_master_grads_case(T, B, False, F, H)


# ---- (e) the slab reductions without a GEMM behind them ------------------------------------------------------------
NWG_SHAPES = [(3, 2033), (4, 2049), EVEN_B, (2, 4097)]        # 128 workgroups (the last ragged), 129, 130, 257
NWG_SHAPES_16 = [(3, 2048), (4, 2064), EVEN_B, (2, 4112)]     # the same counts in whole tiles (path 1's H=128 backward)
# (id, H, rank, kernel path, shapes): path 2 under FLAG_SAVE_PREACT; path 1 as tests/test_hip_parity.py runs it
SLAB_ROUTES = [("dense128", 128, None, 2, NWG_SHAPES), ("lowrank256", 256, 16, 2, NWG_SHAPES),
               ("f32mfma128", 128, None, 1, NWG_SHAPES_16), ("f32mfma64", 64, None, 1, NWG_SHAPES)]
SLAB_CASES = [pytest.param(H, rank, path, T, B, id="%s-%d-%d" % (name, T, B))
              for name, H, rank, path, shapes in SLAB_ROUTES for T, B in shapes]


@pytest.mark.parametrize("H,rank,path,T,B", SLAB_CASES)
def test_slab_reductions_across_their_rounds(H, rank, path, T, B):
    """Every weight gradient is a slab sum here, by the one fixed_order_sum of kws_amd/csrc/scan_common.h: dense
    H=128 / F=32 (reduce_slabs_split, 8 loads per round: rounds of 128 workgroups), low-rank H=256
    (reduce_lowrank_slabs, 4 loads: rounds of 64) and path 1's reduce_slabs (8 loads) at H=128 and H=64 under
    FLAG_FORCE_F32_MFMA with the reference's saved pair; one, two and three rounds, the last one guarded.  Path 1's
    H=128 backward takes whole tiles only (mfma_supported), so it gets the same workgroup counts with B % 16 == 0.
    Bounds of tests/test_hip_fullsize.py; path 1's scalar sums are not compensated, so d_zeta / d_nu get
    SCALAR_TERM_TOL as in section (b)."""
    F = 32
    for shapes in (NWG_SHAPES, NWG_SHAPES_16):
        assert [-(-b // 16) for _, b in shapes] == [128, 129, 130, 257]
        assert [PC.slab_rounds(-(-b // 16), 128)[0] for _, b in shapes] == [1, 2, 2, 3]
    assert all(b % 16 == 0 for _, b in NWG_SHAPES_16)
    rng = np.random.default_rng(600 + B + H)
    p = O.make_params(F, H, rank, rank, np.float32, seed=61, randomize_scalars=True)
    x = rng.standard_normal((T, B, F)).astype(np.float32)
    G = rng.standard_normal((T, B, H)).astype(np.float32)
    h0 = (0.5 * rng.standard_normal((B, H))).astype(np.float32)
    P = S.cell_tensors(p)
    xt, Gt, ht = S.to_dev(x), S.to_dev(G), S.to_dev(h0)
    flags = _lib.FLAG_SAVE_PREACT if path == 2 else _lib.FLAG_FORCE_F32_MFMA
    r = rank or 0
    assert fastgrnn_cuda.kernel_path(T, B, F, H, r, r, direction=0, flags=flags) == path
    assert fastgrnn_cuda.kernel_path(T, B, F, H, r, r, direction=1, flags=flags) == path
    outs, gr = S.fwd_bwd(xt, ht, Gt, P, "sigmoid", flags=flags, biases=path == 2)
    torch.cuda.synchronize()
    hs_o, _, _, g_o = S.oracle64(x, G, p, h0)
    assert np.abs(outs[0].cpu().numpy() - hs_o).max() <= 1e-5
    errs = S.check_grads(gr, g_o, tol=2e-5, scalar_term_tol=0.0 if path == 2 else S.SCALAR_TERM_TOL,
                         tag=(H, rank, path, T, B))
    print("slabs H=%d rank=%s path=%d T=%d B=%d: %s" % (H, rank, path, T, B, {k: "%.1e" % v for k, v in errs.items()}))


# ---- (f) the BatchNorm trainer -------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,B", [(5, 1645), EVEN_B], ids=_ids)
@pytest.mark.parametrize("H,F", [(256, 32), (128, 64)], ids=_ids)
def test_batchnorm_trainer_on_multi_stage_chunks(H, F, T, B):
    """fastgrnn_hip_bn_train_* (its weight gradients are tn_gemm_big_run products over R and R - B rows) at a shape with
    a one-row last stage and one with B a multiple of 32, under the bound of tests/test_hip_bn_train.py"""
    worst = BN.compare(BN.random_case(F, H, T, B, "sigmoid", seed=900 + H + F + B))
    print("bn_train H=%d F=%d T=%d B=%d: worst error / bound %.2f" % (H, F, T, B, worst))
