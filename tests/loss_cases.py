"""Shared by tests/test_losses_math.py and tests/test_gpu_losses.py: the seeded inputs of the loss tests (xdet/losses.py) and
the float yardstick.  Anchors and ground truth come from tests/target_cases.py.

RPN cases: (cls [N,n,2A], loc [N,n,4A], labels [N,n*A], targets [N,n*A,4], anchors_per_image, fg_ratio, seed).  The large
ones take their labels from a seeded draw with the class frequencies of an encoded batch (encoding 128 images on the host
would take minutes); the small ones are encoded from target_cases' ground truth.
Head cases: (cls [N,P,C], reg [N,P,4], labels [N,P], targets [N,P,4], fg_ratio, ohem_k).  As ext_encode_rois' up-sampling
produces them, rows are repeated: in image n the base row with the largest loss appears three times and the next ones twice,
so that for an even K inside that region the K-th and (K+1)-th largest are one row's two copies."""
import numpy as np

import target_cases as C

f32 = np.float32
A = 22
N_A = {64: 4 * 4 * A, 480: 30 * 30 * A, 800: 50 * 50 * A}       # input size -> anchors per image (stride 16)


def distance(got, want64):
    """largest |got - want| / max(1, |want|)"""
    got, want64 = np.asarray(got, np.float64), np.asarray(want64, np.float64)
    if got.size == 0:
        return 0.
    return float((np.abs(got - want64) / np.maximum(1., np.abs(want64))).max())


# ---- RPN -------------------------------------------------------------------------------------------------------------

def _rpn_inputs(rng, labels):
    N, n_a = labels.shape
    cls = (3. * rng.standard_normal((N, n_a // A, 2 * A))).astype(f32)
    loc = (0.8 * rng.standard_normal((N, n_a // A, 4 * A))).astype(f32)
    targets = (0.8 * rng.standard_normal((N, n_a, 4))).astype(f32) * (labels > 0)[..., None].astype(f32)
    return cls, loc, labels.astype(np.int32), targets


def _drawn_labels(rng, N, n_a, n_pos, n_neg):
    """exactly n_pos labels > 0 and n_neg labels == 0 in the batch, the rest -1"""
    lab = np.full(N * n_a, -1, np.int32)
    where = rng.permutation(N * n_a)[:n_pos + n_neg]
    lab[where[:n_pos]] = rng.integers(1, 21, n_pos)
    lab[where[n_pos:]] = 0
    return lab.reshape(N, n_a)


def _encoded_labels(seed, N, size):
    from xdet import targets as T
    anchor = C.anchors(size)
    labels, boxes = C.make_ground_truth(seed, N, anchor)
    l, t, _ = T.host_encode_anchors(anchor, labels, boxes)
    return l, t


RPN_CASES = {
    # name: (N, size, (n_pos, n_neg) or None = encoded from ground truth, anchors_per_image, fg_ratio, seed)
    'down_both_128x480': (128, 480, (25000, 2000000), 256, 0.25, 11),
    'short_pos': (8, 480, (100, 120000), 256, 0.25, 12),
    'short_neg_tail': (4, 480, (50, 300), 256, 0.25, 13),
    'tail_whole': (2, 480, (16, 48), 256, 0.25, 14),
    'no_pos': (2, 480, (0, 30000), 256, 0.25, 15),
    'nothing': (2, 480, (0, 0), 256, 0.25, 16),
    'pos_only_exact': (2, 480, (128, 0), 256, 0.25, 17),
    'encoded_n1': (1, 480, None, 256, 0.25, 18),
    'encoded_n4_half': (4, 480, None, 64, 0.5, 19),
    'set_800': (16, 800, (9000, 700000), 256, 0.25, 20),
    # S = 32768 of M = 45056 anchors: ~3000 selected keys per 4096-anchor chunk, more than a workgroup of the compaction stages
    'dense_128x64': (128, 64, (12000, 30000), 256, 0.25, 21),
}


def rpn_case(name):
    N, size, draw, api, fg, seed = RPN_CASES[name]
    rng = np.random.default_rng(1000 + seed)
    if draw is None:
        labels, targets = _encoded_labels(seed, N, size)
        cls, loc, labels, _ = _rpn_inputs(rng, labels)
    else:
        cls, loc, labels, targets = _rpn_inputs(rng, _drawn_labels(rng, N, N_A[size], *draw))
    return cls, loc, labels, targets, api, fg, seed


def anchor_major(x, c):
    """[N,n,c*A] in the net's layout -> [N*n*A, c]: row (pixel * A + k)"""
    return np.asarray(x).reshape(-1, c)


# ---- head ------------------------------------------------------------------------------------------------------------

HEAD_CASES = {
    # name: (N, P, C, ohem_k, seed, logit range (lo, hi) or None = 2.5 * normal, images whose rows are all label -1)
    'ohem_k_lt_p': (8, 64, 21, 32, 3, None, ()),
    'ohem_k_ge_p': (2, 64, 21, 100, 1, None, ()),
    'no_ohem': (4, 64, 21, 0, 3, None, ()),
    'image_all_ignored': (3, 64, 21, 16, 1, None, (1,)),
    'logits_to_50': (2, 64, 21, 32, 1, (-30., 50.), ()),
    'p256': (2, 256, 21, 128, 361, None, ()),
}
FG_RATIO = 0.25


def head_case(name):
    return build_head_case(*HEAD_CASES[name])


def build_head_case(N, P, Cn, k, seed, rng_range=None, ignored=()):
    from xdet import losses as L
    rng = np.random.default_rng(2000 + seed)
    K = min(k, P) if k > 0 else P
    n_dup = min(K // 2 + 3, P // 3)               # base rows that are repeated; the first of them twice
    B = P - n_dup - 1
    cls, reg = np.zeros((N, P, Cn), f32), np.zeros((N, P, 4), f32)
    labels, targets = np.zeros((N, P), np.int32), np.zeros((N, P, 4), f32)
    for n in range(N):
        if rng_range is None:
            c = (2.5 * rng.standard_normal((B, Cn))).astype(f32)
        else:
            c = rng.uniform(rng_range[0], rng_range[1], (B, Cn)).astype(f32)
        r = (0.8 * rng.standard_normal((B, 4))).astype(f32)
        l = np.where(rng.random(B) < 0.25, rng.integers(1, Cn, B), 0).astype(np.int32)
        t = (0.8 * rng.standard_normal((B, 4))).astype(f32) * (l > 0)[:, None].astype(f32)
        per = L.host_head_loss(c[None], r[None], l[None], t[None], FG_RATIO).per_roi[0]
        top = np.argsort(-per, kind='stable')[:n_dup]
        src = np.concatenate([np.arange(B), top[:1], top])                  # B + 1 + n_dup = P rows
        src = src[rng.permutation(P)]                                        # the copies lie anywhere among the rows
        cls[n], reg[n], labels[n], targets[n] = c[src], r[src], l[src], t[src]
        if n in ignored:
            labels[n], targets[n] = -1, 0.
    return cls, reg, labels, targets, FG_RATIO, k


def duplicate_groups(cls, reg, labels, targets):
    """per image: group id of every row; rows with bit-equal inputs share one"""
    N, P = labels.shape
    out = np.zeros((N, P), np.int64)
    for n in range(N):
        rows = np.concatenate([cls[n].view(np.uint32), reg[n].view(np.uint32), labels[n][:, None].astype(np.uint32),
                               targets[n].view(np.uint32)], 1)
        _, out[n] = np.unique(rows, axis=0, return_inverse=True)
    return out
