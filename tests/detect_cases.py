"""Cases shared by tests/test_detect_cpu.py and tests/test_hip_detect.py: the detector's vote restated in plain Python,
and the seeded operands of the inference head with their fp64 reference.  Not a test file.

The vote (include/fastgrnn_hip.h, fastgrnn_hip_vote_windows), per stream, from an empty vote list and
no previous detection.  For window w:
  votes    = pred[max(0, w-K+1) .. w]
  (m, f)   = the most frequent value in votes and its frequency; on equal frequency the value whose first occurrence
             in votes is earliest (Counter(votes).most_common(1): insertion order, first maximum)
  majority = m if f >= M else -1
  event    = m if f >= M and m != previous else -1; previous becomes m when an event fires
A negative entry of pred is a vote for no class: it occupies its slot in the list and is never m.
"""
import collections
import functools

import torch

VOTE_CHUNK = 256          # windows per pass of the kernel's workgroup (kernels_head.hip; held to it in test_detect_cpu)


def vote_reference(pred, K, M):
    """pred: a list of ints (one stream) -> (majority, event), two lists of the same length."""
    votes, previous = [], None
    majority, event = [], []
    for p in pred:
        if len(votes) == K:
            votes.pop(0)
        votes.append(int(p))
        maj = ev = -1
        counted = collections.Counter(v for v in votes if v >= 0).most_common(1)
        if counted:
            m, f = counted[0]
            if f >= M:
                maj = m
                if m != previous:
                    ev = m
                    previous = m
        majority.append(maj)
        event.append(ev)
    return majority, event


def vote_reference_streams(pred, K, M):
    """pred: [S][Nw] nested lists -> (majority, event) as nested lists; the streams are independent."""
    out = [vote_reference(row, K, M) for row in pred]
    return [o[0] for o in out], [o[1] for o in out]


# ---- typed-out cases: (name, pred, K, M, majority, event) -------------------------------------------------------------
A_, B_ = 1, 2
TYPED_CASES = [
    # five against five: A entered the list first, so A is the majority at the tenth window (no majority before it)
    ("tie_5_5_A_first", [A_, B_] * 5, 10, 5, [-1] * 8 + [A_, A_], [-1] * 8 + [A_, -1]),
    # the same list one window later: A's first vote has left the list, B is now the older of the two, and at 5:5 B wins
    ("tie_5_5_shifted", [A_, B_] * 5 + [A_], 10, 5, [-1] * 8 + [A_, A_, B_], [-1] * 8 + [A_, -1, B_]),
    ("tie_5_5_B_first", [B_, A_] * 5, 10, 5, [-1] * 8 + [B_, B_], [-1] * 8 + [B_, -1]),
    # a negative vote occupies a slot: K = 3, the list at the last window is [-1, 3, -1], one vote for 3 only
    ("negative_holds_a_slot", [3, 3, -1, 3, -1], 3, 2, [-1, 3, 3, 3, -1], [-1, 3, -1, -1, -1]),
    # ... and is never the majority, however frequent
    ("negative_is_never_m", [-5, -5, -5, 2], 4, 1, [-1, -1, -1, 2], [-1, -1, -1, 2]),
    # an event fires only on change
    ("event_once", [4, 4, 4], 3, 2, [-1, 4, 4], [-1, 4, -1]),
    # no event before M votes exist
    ("needs_M_votes", [7, 7, 7, 7, 7, 7], 10, 5, [-1, -1, -1, -1, 7, 7], [-1, -1, -1, -1, 7, -1]),
    # previous survives windows without a majority: 1 is reported once, 2 once, then 1 again
    ("previous_is_kept", [1, 1, 2, 0, 2, 2, 0, 1, 1], 2, 2, [-1, 1, -1, -1, -1, 2, -1, -1, 1], [-1, 1, -1, -1, -1, 2, -1, -1, 1]),
    ("previous_same_again", [1, 1, 0, 2, 1, 1], 2, 2, [-1, 1, -1, -1, -1, 1], [-1, 1, -1, -1, -1, -1]),
]


# ---- seeded vote cases: (name, S, Nw, K, M) ----------------------------------------------------------------------------
def _draw(seed, S, Nw):
    """Predictions from 3 classes (majorities and ties are frequent), about one in sixteen negative."""
    g = torch.Generator().manual_seed(seed)
    p = torch.randint(0, 3, (S, Nw), generator=g, dtype=torch.int32)
    neg = torch.randint(0, 16, (S, Nw), generator=g) == 0
    return torch.where(neg, torch.full_like(p, -1), p)


@functools.lru_cache(maxsize=None)
def vote_case(name):
    """-> (pred [S,Nw] int32 CPU tensor, K, M)"""
    if name.startswith("nw"):                                  # S = 3, K = 10, M = 5, Nw around K and M
        nw = int(name[2:])
        p = _draw(100 + nw, 3, nw)
        if nw == 5:
            p[1, :] = 2                                        # five votes exist only at the last window: all five agree
        return p, 10, 5
    if name == "k1":
        return _draw(7, 2, 40), 1, 1
    if name == "k64":
        # 33 of 64 needs a biased stream (uniform draws from 3 classes never get there).  Stream 0: class 1 at 3 in 4
        # for 70 windows (a majority inside the first 64, while the list is still filling), then class 2 at 3 in 4 (the
        # majority lapses, then changes, with all 63 predecessors in play).  Stream 1: 1,2 alternating for 64 windows
        # (32:32, one vote short), then a run of 1 (33 votes only once the list is full), then a run of 0.
        p = _draw(8, 2, 200)
        g = torch.Generator().manual_seed(18)
        keep = torch.randint(0, 4, (200,), generator=g) != 0
        p[0, :70] = torch.where(keep[:70] & (p[0, :70] >= 0), torch.ones_like(p[0, :70]), p[0, :70])
        p[0, 70:] = torch.where(keep[70:] & (p[0, 70:] >= 0), torch.full_like(p[0, 70:], 2), p[0, 70:])
        p[1, :64] = torch.tensor([1, 2] * 32, dtype=torch.int32)
        p[1, 64:110] = 1
        p[1, 110:] = 0
        return p, 64, 33
    if name == "k64_ties":
        # K = 64, M = 32: 1,2 alternating holds a 32:32 tie at every window from the 64th on, and the value that is older
        # in the list changes with every window -- the first-occurrence rule at the largest K, an event per window; then
        # uniform draws
        p = _draw(19, 1, 150)
        p[0, :100] = torch.tensor([1, 2] * 50, dtype=torch.int32)
        return p, 64, 32
    if name in ("chunk_plus_1", "two_chunks_plus_3"):
        # a long run of qualifying majorities (class 1) ends just before each chunk boundary: the chunk's last window has
        # no majority (four votes), and the next chunk's first window has one again -- its `previous` is the carried value
        nw = VOTE_CHUNK + 1 if name == "chunk_plus_1" else 2 * VOTE_CHUNK + 3
        p = _draw(9 if name == "chunk_plus_1" else 10, 2, nw)
        for edge in range(VOTE_CHUNK, nw, VOTE_CHUNK):
            p[:, edge - 60:edge - 10] = 1
            p[0, edge - 10:edge + 1] = torch.tensor([0, 1, 1, 1, 1, 0, 2, -1, 0, 2, 1], dtype=torch.int32)   # 1 again: no event
            p[1, edge - 10:edge + 1] = torch.tensor([0, 2, 2, 2, 2, 0, 1, -1, 0, 1, 2], dtype=torch.int32)   # 2: an event
        return p, 10, 5
    if name == "leak":
        # stream 0 ends in nine votes for 2; stream 1 begins with one: a leak would give stream 1 a majority at once
        p = _draw(11, 2, 30)
        p[0, -9:] = 2
        p[1, :4] = 2
        return p, 10, 5
    raise KeyError(name)


VOTE_CASES = ["nw1", "nw4", "nw5", "nw9", "nw10", "nw11", "k1", "k64", "k64_ties", "chunk_plus_1", "two_chunks_plus_3", "leak"]


# ---- the inference head ------------------------------------------------------------------------------------------------
HEAD_SHAPES = [(1, 64, 2), (37, 128, 12), (130, 20, 64), (33, 256, 64), (4097, 128, 12)]
# a row is excused from pred == fp64 argmax when its two largest fp64 logits are closer than this share of the largest
# logit magnitude; the seeds below are chosen so that no row is (asserted in tests/test_detect_cpu.py)
GAP_BOUND = 2e-5
HEAD_SEEDS = {(1, 64, 2): 41, (37, 128, 12): 41, (130, 20, 64): 41, (33, 256, 64): 42, (4097, 128, 12): 42}


@functools.lru_cache(maxsize=None)
def head_case(B, H, Cn, tie=False):
    """Seeded operands (drawn as tests/test_hip_parity.py draws the training head's) and their fp64 reference, computed
    once: dict with h, w, b (fp32), y (int64, a few -100), logits64, logp64, argmax64, excused (bool [B]).  ``tie``:
    class rows 3 and 7 of w and b are identical."""
    g = torch.Generator().manual_seed(HEAD_SEEDS[B, H, Cn])
    h = torch.randn(B, H, generator=g)
    w = 0.3 * torch.randn(Cn, H, generator=g)
    b = 0.1 * torch.randn(Cn, generator=g)
    y = torch.randint(0, Cn, (B,), generator=g)
    if tie:
        w[7], b[7] = w[3], b[3]
    logits = h.double() @ w.double().t() + b.double()
    am = logits.argmax(dim=1)
    # (half of the labels are made right, so that the count is not a handful; a few rows are ignored)
    y = torch.where(torch.arange(B) % 2 == 0, am, y)
    y[::7] = -100
    if Cn > 1:
        top2 = logits.topk(2, dim=1).values
        excused = (top2[:, 0] - top2[:, 1]) < GAP_BOUND * logits.abs().max()
    else:
        excused = torch.zeros(B, dtype=torch.bool)
    return {"h": h, "w": w, "b": b, "y": y, "logits64": logits, "logp64": torch.log_softmax(logits, dim=1),
            "argmax64": am, "excused": excused}
