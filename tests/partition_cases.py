"""How the GEMMs and slab reductions around the scans cut their work, restated in Python, and the (T, B) shapes at
which the GPU tests of tests/test_hip_partition_seams.py run them.

R = T * B rows of a time-major sequence, nwg = ceil(B / 16) workgroups of a scan.  Three rules are restated here, each
from the launcher it quotes; tests/test_partition_cases_cpu.py holds the restatement to the library (the TN rule through
the workspace the library asks for) and asserts that the table below covers every class in CLASSES.

  rows GEMM   kws_amd/csrc/kernels_gemm.hip, launch_rows_gemm / launch_rows_gemm_bft / rows_gemm_split:
              stages of RG_ROWS = 32 rows; nwg = min(nstages, 256) workgroups; spw = ceil(nstages / nwg) consecutive
              stages each; workgroup i runs stages [i * spw, min((i + 1) * spw, nstages)) and leaves at once when that
              range is empty.
  TN GEMM     kws_amd/csrc/kernels_gemm.hip, tnb_chunks / tn_gemm_big_run / tn_big_reduce:
              stages of TNB_STAGE = 32 rows; want = min(256 / nblk, nstages) chunks with nblk = M / 128 column blocks;
              spw = ceil(nstages / want); nch = ceil(nstages / spw); the grid is ceil(nch / 8) * 8 * nblk workgroups,
              those with chunk >= nch leave; tn_big_reduce sums nch partials (with bf16 sequences and 0 < shiftB < R the
              partials of the body over R - shiftB rows, then those of the fp32 head over shiftB rows).
  slab sums   kws_amd/csrc/scan_common.h, fixed_order_sum<W>: 16 groups x W partials per round, the outer loop strides
              by 16 * W; the last round is guarded partial by partial.  Its callers fix W: 8 (stride 128 workgroups) in
              reduce_slabs_split (kernels_split.hip) and reduce_slabs (kernels_mfma.hip), 4 (stride 64) in
              reduce_h256_small (kernels_h256.hip), reduce_lowrank_slabs (kernels_lowrank.hip) and, over chunks,
              tn_big_reduce (kernels_gemm.hip).
"""
from collections import namedtuple

STAGE = 32                # RG_ROWS and TNB_STAGE
MAX_WG = 256              # one workgroup per CU
TN_GRID_PAD = 8           # tn_gemm_big_run: dim3 grid(((nch + 7) / 8) * 8 * nblk)
SLAB_STRIDE = {128: 128, 256: 64}      # hidden size -> workgroups per round of its slab reduction

Cut = namedtuple("Cut", "nstages spw nchunk last idle")    # last: stages of the last chunk; idle: workgroups with no stage


def _ceil(a, b):
    return -(-a // b)


def rows_gemm_cut(R):
    """launch_rows_gemm: (nstages, stages per workgroup, active workgroups, stages of the last active one, idle ones)"""
    nstages = _ceil(R, STAGE)
    nwg = min(nstages, MAX_WG)
    spw = _ceil(nstages, nwg)
    active = _ceil(nstages, spw)               # rows_gemm_split: workgroups with s_begin < nstages
    return Cut(nstages, spw, active, nstages - (active - 1) * spw, nwg - active)


def tn_cut(R, nblk):
    """tnb_chunks: (nstages, stages per chunk, nch, stages of the last chunk, padded workgroups per column block)"""
    nstages = _ceil(R, STAGE)
    want = max(1, min(MAX_WG // nblk, nstages))
    spw = _ceil(nstages, want)
    nch = _ceil(nstages, spw)
    return Cut(nstages, spw, nch, nstages - (nch - 1) * spw, _ceil(nch, TN_GRID_PAD) * TN_GRID_PAD - nch)


def tn_partials(R, nblk, shift=0, bf16=False):
    """tn_gemm_big_run: partials tn_big_reduce sums -- (body, head); head is 0 unless bf16 rows meet an fp32 h0"""
    if bf16 and 0 < shift < R:
        return tn_cut(R - shift, nblk).nchunk, tn_cut(shift, nblk).nchunk
    return tn_cut(R, nblk).nchunk, 0


def tn_slots(R, nblk):
    """tn_gemm_big_ws: partials the workspace has room for"""
    return 2 * tn_cut(R, nblk).nchunk


def slab_rounds(nwg, stride):
    """(rounds of the outer loop, workgroups in the last one)"""
    rounds = _ceil(nwg, stride)
    return rounds, nwg - (rounds - 1) * stride


def seam_utterances(T, B):
    """Utterances (time-major: row r = t * B + b) whose rows sit on either side of the first and of the last chunk
    boundary of each cut, with b = 0 and b = B - 1."""
    R = T * B
    bs = {0, B - 1}
    for cut in (rows_gemm_cut(R), tn_cut(R, 1), tn_cut(R, 2)):
        for edge in (cut.spw * STAGE, (cut.nchunk - 1) * cut.spw * STAGE):
            if 0 < edge < R:
                bs.update(((edge - 1) % B, edge % B))
    return sorted(bs)


# (T, B, what the shape is there for)
TABLE = [
    (3, 2731, "257 stages: chunks of 2, last of 1 holding one row; 127 idle rows-GEMM workgroups; M=256: 3, last 2"),
    (5, 1645, "258 stages: last chunk full (2), tail 1"),
    (5, 3289, "514 stages: chunks of 3 (M=256: 5, last 4), last of 1, tail 29"),
    (11, 1499, "516 stages: chunks of 3 all full; M=256: chunks of 5, last of 1"),
    (5, 2080, "B mod 32 = 0: the w4 dU route at 2-3 stages per chunk, no tail, nwg = 130"),
    (3, 2752, "B mod 32 = 0, 258 stages"),
    (99, 83, "the workload's T with an epoch's last batch: B mod 32 = 19, tail 25"),
    (2, 4097, "nwg = 257: third round of the slab reductions"),
    (3, 2033, "nwg = 128 with a ragged last workgroup; one stage per chunk, TN padding 1"),
    (4, 2049, "nwg = 129"),
    (7, 3519, "770 stages: chunks of 4, last of 2, tail 25; M=256: chunks of 7, all full"),
    (8, 3088, "772 stages: chunks of 4 all full, B mod 32 = 16"),
    (9, 3647, "1026 stages: chunks of 5, last of 1, tail 23 (below 25: the tail class is met elsewhere)"),
    (10, 3296, "1030 stages: chunks of 5 all full, B mod 32 = 0"),
    (2, 3200, "200 stages: M=256 chunks of 2 all full, B mod 32 = 0"),
    (3, 4117, "386 stages: M=256 chunks of 4, last of 2; tail 31"),
    (4, 3104, "388 stages: M=256 chunks of 4 all full, B mod 32 = 0"),
    (5, 3295, "515 stages: M=256 chunks of 5 all full; M=128: chunks of 3, last of 2"),
    (2, 1500, "94 stages: one stage per chunk at M=256 too"),
]
SHAPES = [(T, B) for T, B, _ in TABLE]
MAX_ROWS = 50000

CLASSES = (
    ["%s chunks of %d" % (fam, n) for fam in ("rows", "tn1", "tn2") for n in (1, 2, 3, 4, 5)]
    + ["%s chunks of %d, last %s" % (fam, n, k) for fam in ("rows", "tn1", "tn2") for n in (2, 3, 4, 5)
       for k in ("short", "full")]
    + ["tail 0", "tail 1 in a multi-stage chunk", "tail >= 25 in a multi-stage chunk",
       "idle rows-GEMM workgroups", "TN padding 7",
       "w4 dU route, multi-stage (x2)", "mixed-stage dU route, multi-stage (x3)",
       "nwg 127/128 ragged", "nwg 129", "nwg 257"])


def classes_of(T, B):
    """The classes of CLASSES that the shape (T, B) exercises (the two counted ones without their count)."""
    R = T * B
    out = set()
    cuts = {"rows": rows_gemm_cut(R), "tn1": tn_cut(R, 1), "tn2": tn_cut(R, 2)}
    for fam, c in cuts.items():
        if c.spw <= 5:
            out.add("%s chunks of %d" % (fam, c.spw))
            if c.spw >= 2 and c.nchunk > 1:
                out.add("%s chunks of %d, last %s" % (fam, c.spw, "short" if c.last < c.spw else "full"))
    tail = R % STAGE
    # (the tail sits in the last chunk: it is inside a multi-stage chunk when that chunk has two stages or more)
    multi_last = any(c.last >= 2 for c in cuts.values())
    if tail == 0:
        out.add("tail 0")
    if tail == 1 and multi_last:
        out.add("tail 1 in a multi-stage chunk")
    if tail >= 25 and multi_last:
        out.add("tail >= 25 in a multi-stage chunk")
    if cuts["rows"].idle > 0:
        out.add("idle rows-GEMM workgroups")
    if 7 in (cuts["tn1"].idle, cuts["tn2"].idle):
        out.add("TN padding 7")
    # dU = d_pre^T . H_prev of the H = 256 layer (M = 256, N = 256, shiftB = B): tn_gemm_big_run's choice
    if cuts["tn2"].spw >= 2:
        out.add("w4 dU route, multi-stage" if B % STAGE == 0 else "mixed-stage dU route, multi-stage")
    nwg = _ceil(B, 16)
    if nwg in (127, 128) and B % 16:
        out.add("nwg 127/128 ragged")
    if nwg in (129, 257):
        out.add("nwg %d" % nwg)
    return out


def coverage(shapes=None):
    """class -> the shapes of the table that exercise it"""
    cov = {c: [] for c in CLASSES}
    for T, B in (SHAPES if shapes is None else shapes):
        for c in classes_of(T, B):
            for name in (c, c + " (x2)", c + " (x3)"):
                if name in cov:
                    cov[name].append((T, B))
    return cov


def missing(shapes=None):
    need = {"w4 dU route, multi-stage (x2)": 2, "mixed-stage dU route, multi-stage (x3)": 3}
    return sorted(c for c, s in coverage(shapes).items() if len(s) < need.get(c, 1))
