"""The training-loss contract (include/xdet.h "training losses") without a GPU: the vectorised NumPy
statement of xdet/losses.py against a loop-per-row restatement written here from the contract's text, its gradients against
central differences of its own float64 loss, the selection against targets.sample_rois, the input conditions the GPU tests
rely on, and the argument errors.

The f32 statement's own distance from the float64 one over all cases of tests/loss_cases.py (the GPU tests' bar is four
times this; printed by test_f32_statement_distance_from_float64): 2.3e-07 relative to max(1, |value|)."""
import math

import numpy as np
import pytest

import loss_cases as LC

f32 = np.float32
SMALL_RPN = ('short_neg_tail', 'tail_whole', 'no_pos', 'nothing', 'pos_only_exact', 'encoded_n1', 'encoded_n4_half')


# ---- the restatement: one row at a time, Python floats ---------------------------------------------------------------

def loop_sl1(d, sigma=1.):
    s2 = sigma * sigma
    return 0.5 * s2 * d * d if abs(d) < 1. / s2 else abs(d) - 0.5 / s2


def loop_ce(x, y):
    m = max(x)
    return math.log(sum(math.exp(v - m) for v in x)) - (x[y] - m)


def loop_select(labels, S, fg_ratio, seed):
    """select_samples over the flat labels -> (rows [S] or [-1] * S, counts)"""
    from xdet import targets as T
    pos = [i for i, l in enumerate(labels) if l > 0]
    neg = [i for i, l in enumerate(labels) if l == 0]

    def shuffled(elems, stream):
        keys = T.shuffle_keys(seed, 0, np.asarray(elems, np.int64), stream).tolist() if elems else []
        return [e for _, e in sorted(zip(keys, elems))]
    exp_fg = int(np.rint(f32(S) * f32(fg_ratio)))
    fg = pos if len(pos) < exp_fg else shuffled(pos, 0)[:exp_fg]
    exp_bg = S - min(len(pos), exp_fg)
    bg = neg if len(neg) < exp_bg else shuffled(neg, 0)[:exp_bg]
    keep = fg + bg
    if not keep:
        return [-1] * S, (len(pos), len(neg), 0)
    if len(keep) < S:
        left = S - len(keep)
        order = list(range(len(keep))) * (left // len(keep) + 1) + shuffled(list(range(len(keep))), 1)[:left % len(keep)]
        rows = [keep[p] for p in order]
    else:
        rows = keep
    assert len(rows) == S
    return rows, (len(pos), len(neg), len(keep))


def loop_rpn(cls, loc, labels, targets, S, fg_ratio, seed):
    rows, (n_pos, n_neg, n_keep) = loop_select(labels.tolist(), S, fg_ratio, seed)
    if n_keep == 0:
        return rows, (n_pos, n_neg, 0, 0), (0., 0., 0.)
    cls, loc, targets = cls.astype(np.float64).tolist(), loc.astype(np.float64).tolist(), targets.astype(np.float64).tolist()
    ce, l1, n_sel_pos = 0., 0., 0
    for r in rows:
        y = 1 if labels[r] > 0 else 0
        ce += loop_ce(cls[r], y)
        if y:
            n_sel_pos += 1
            l1 += sum(loop_sl1(loc[r][k] - targets[r][k]) for k in range(4))
    ce /= S
    l1 = l1 / n_sel_pos / fg_ratio if n_sel_pos else 0.
    return rows, (n_pos, n_neg, n_keep, n_sel_pos), (ce, l1, ce + l1)


def loop_head(cls, reg, labels, targets, fg_ratio, ohem_k):
    N, P, Cn = cls.shape
    per = np.zeros((N, P))
    parts = np.zeros((N, P, 2))
    for n in range(N):
        for p in range(P):
            l = int(labels[n, p])
            if not 0 <= l < Cn:
                continue
            ce = loop_ce(cls[n, p].astype(np.float64).tolist(), l)
            l1 = sum(loop_sl1(float(reg[n, p, k]) - float(targets[n, p, k])) for k in range(4)) / fg_ratio if l > 0 else 0.
            per[n, p], parts[n, p] = ce + l1, (ce, l1)
    K = min(ohem_k, P) if ohem_k > 0 else P
    select = [sorted(range(P), key=lambda p: (-per[n, p], p))[:K] if ohem_k > 0 else list(range(P)) for n in range(N)]
    tot = [sum(per[n, p] for n in range(N) for p in select[n]) / (N * K)]
    tot += [sum(parts[n, p, c] for n in range(N) for p in select[n]) / (N * K) for c in (0, 1)]
    return per, np.array(select), tot


@pytest.mark.parametrize('name', SMALL_RPN)
def test_rpn_statement_equals_the_loop(name):
    from xdet import losses as L
    cls, loc, labels, targets, api, fg, seed = LC.rpn_case(name)
    S = labels.shape[0] * api
    rows, counts, losses = loop_rpn(LC.anchor_major(cls, 2), LC.anchor_major(loc, 4), labels.reshape(-1), targets.reshape(-1, 4), S, fg, seed)
    for dtype, tol in ((np.float64, 1e-12), (f32, 1e-5)):
        got = L.host_rpn_loss(LC.anchor_major(cls, 2), LC.anchor_major(loc, 4), labels, targets, api, fg, seed, dtype=dtype)
        assert got.sel_index.tolist() == rows and tuple(got.counts) == counts, name
        assert np.allclose(got.losses, losses, rtol=tol, atol=tol), (name, got.losses, losses)
        # multiplicities: the gradient of a row selected m times is m times that of one selection
        rows_u, mult = np.unique([r for r in rows if r >= 0], return_counts=True)
        assert np.array_equal(np.flatnonzero(np.abs(got.grad_cls).sum(1) > 0), rows_u)
        if len(rows_u):
            left = S - counts[2]
            assert set(mult.tolist()) <= {left // counts[2] + 1, left // counts[2] + 2}


def test_rpn_cases_meet_their_names():
    """an input condition of the GPU tests: every case reaches the branch of the selection it is named after, by the counts
    the NumPy statement reports"""
    from xdet import losses as L
    seen = {}
    for name in SMALL_RPN + ('short_pos', 'dense_128x64'):
        cls, loc, labels, targets, api, fg, seed = LC.rpn_case(name)
        p, q, k, _ = L.host_rpn_loss(LC.anchor_major(cls, 2), LC.anchor_major(loc, 4), labels, targets, api, fg, seed).counts
        seen[name] = (int(p), int(q), int(k), labels.shape[0] * api)
    p, q, k, S = seen['dense_128x64']
    assert k == S and p >= 0.25 * S and q >= 0.75 * S and S * 4096 > 1536 * 128 * LC.N_A[64]     # both down-sampled, > 1536 keys per chunk
    assert seen['short_pos'][0] < 0.25 * seen['short_pos'][3] and seen['short_pos'][2] == seen['short_pos'][3]
    p, q, k, S = seen['short_neg_tail']
    assert 0 < k < S and (S - k) % k != 0
    p, q, k, S = seen['tail_whole']
    assert 0 < k < S and (S - k) % k == 0
    assert seen['no_pos'][0] == 0 and seen['no_pos'][2] > 0 and seen['nothing'][2] == 0
    assert seen['pos_only_exact'][0] == round(0.25 * seen['pos_only_exact'][3]) and seen['pos_only_exact'][1] == 0
    _, _, labels, _, _, _, _ = LC.rpn_case('encoded_n4_half')
    assert (labels == -1).any() and (labels > 0).any()


@pytest.mark.parametrize('name', sorted(LC.RPN_CASES))
def test_rpn_selection_is_sample_rois_on_the_flat_labels(name):
    from xdet import losses as L, targets as T
    cls, loc, labels, targets, api, fg, seed = LC.rpn_case(name)
    S = labels.shape[0] * api
    got = L.host_rpn_loss(LC.anchor_major(cls, 2), LC.anchor_major(loc, 4), labels, targets, api, fg, seed)
    idx, (p, q, k) = T.sample_rois(labels.reshape(-1), np.ones(labels.size, f32), S, fg, 0., seed, image=0)
    assert np.array_equal(got.sel_index, idx) and tuple(got.counts[:3]) == (p, q, k)
    assert got.counts[3] == (labels.reshape(-1)[idx[idx >= 0]] > 0).sum()


@pytest.mark.parametrize('name', sorted(LC.HEAD_CASES))
def test_head_statement_equals_the_loop(name):
    from xdet import losses as L
    cls, reg, labels, targets, fg, k = LC.head_case(name)
    per, select, tot = loop_head(cls, reg, labels, targets, fg, k)
    for dtype, tol in ((np.float64, 1e-12), (f32, 2e-5)):
        got = L.host_head_loss(cls, reg, labels, targets, fg, k, dtype=dtype)
        assert np.array_equal(got.select, select), name
        assert np.allclose(got.per_roi, per, rtol=tol, atol=tol) and np.allclose(got.losses, tot, rtol=tol, atol=tol), name
        on = np.zeros(labels.shape, bool)
        on[np.arange(labels.shape[0])[:, None], select] = True
        assert not got.grad_cls[~on].any() and not got.grad_reg[~on | (labels <= 0)].any()
        assert (np.abs(got.grad_cls[on & (labels >= 0)]).sum(-1) > 0).all()


def test_modified_smooth_l1():
    from xdet import losses as L
    d = np.array([-3., -1., -0.999, -0.25, 0., 0.5, 1., 1.5], f32)
    for sigma in (1., 3.):
        want = [loop_sl1(float(v), sigma) for v in d]
        assert np.allclose(L.modified_smooth_l1(d, np.zeros_like(d), sigma), want, rtol=1e-6)
        assert np.allclose(L.modified_smooth_l1(d, np.zeros_like(d), sigma, np.float64), want, rtol=1e-14)


# ---- gradients ---------------------------------------------------------------------------------------------------------

H, BAR = 1e-5, 1e-8


def central(f, x):
    g = np.zeros_like(x)
    flat, gf = x.reshape(-1), g.reshape(-1)
    for i in range(flat.size):
        keep = flat[i]
        flat[i] = keep + H
        up = f()
        flat[i] = keep - H
        down = f()
        flat[i] = keep
        gf[i] = (up - down) / (2 * H)
    return g


def test_gradients_equal_central_differences():
    """d loss / d logits of the float64 statement against (f(x + h) - f(x - h)) / 2h of its own loss, h = 1e-5, bar 1e-8.
    The loss is O(1) (<= ~10) and a sum of <= 64 terms, so a float64 evaluation carries at most ~64 * 1.1e-16 * 10 = 7e-14
    of rounding, which the difference quotient magnifies by 1 / 2h: <= 4e-9.  The truncation term is h^2 / 6 * |f'''|; the
    cross entropy's third derivative is below 1 and the smooth L1 is quadratic or linear away from |d| = 1 (the test
    requires every |d| to be at least 1e-3 away from it), each scaled by a weight <= 1 / fg_ratio = 4: <= 7e-11.  Together
    below 5e-9 < 1e-8, while a wrong factor (1/S, 1/n_pos, 1/fg_ratio, a multiplicity, the OHEM mask) changes a gradient
    entry by at least its own size, ~1e-3 here."""
    from xdet import losses as L
    rng = np.random.default_rng(7)
    # RPN: 2 images x 40 anchors, S = 32, 3 positives and 9 negatives: tail with multiplicities 2 and 3
    labels = np.full((2, 40), -1, np.int32)
    labels[0, [3, 17]], labels[1, 5] = 4, 9
    labels[0, [1, 2, 30]], labels[1, [0, 7, 8, 9, 20, 33]] = 0, 0
    cls, loc = rng.standard_normal((80, 2)), rng.standard_normal((80, 4))
    tg = rng.standard_normal((80, 4)) * (labels.reshape(-1) > 0)[:, None]
    assert (np.abs(np.abs(loc - tg) - 1.) > 1e-3).all()
    run = lambda: L.host_rpn_loss(cls, loc, labels, tg, 16, 0.25, seed=3, dtype=np.float64)
    res = run()
    assert tuple(res.counts[:3]) == (3, 9, 12) and len(set(np.unique(res.sel_index, return_counts=True)[1])) == 2
    for x, g in ((cls, res.grad_cls), (loc, res.grad_loc)):
        num = central(lambda: float(run().losses[2]), x)
        assert np.abs(num - g).max() < BAR, np.abs(num - g).max()
        assert np.abs(g).max() > 1e-3
    # head: 2 images x 12 ROIs, K = 5 (the mask is a constant of the differentiation: the selection must not move)
    c, r = 2. * rng.standard_normal((2, 12, 6)), rng.standard_normal((2, 12, 4))
    hl = np.where(rng.random((2, 12)) < 0.4, rng.integers(1, 6, (2, 12)), 0)
    hl[1, 4] = -1
    ht = rng.standard_normal((2, 12, 4)) * (hl > 0)[..., None]
    assert (np.abs(np.abs(r - ht) - 1.) > 1e-3).all()
    for k in (5, 0):
        runh = lambda: L.host_head_loss(c, r, hl, ht, 0.25, k, dtype=np.float64)
        res = runh()
        srt = -np.sort(-res.per_roi, 1)
        assert k == 0 or (srt[:, :-1] - srt[:, 1:])[:, :k].min() > 1e-3           # no selection change within h

        def f():
            out = runh()
            assert np.array_equal(out.select, res.select)
            return float(out.losses[0])
        for x, g in ((c, res.grad_cls), (r, res.grad_reg)):
            num = central(f, x)
            assert np.abs(num - g).max() < BAR, (k, np.abs(num - g).max())
            assert np.abs(g).max() > 1e-3


# ---- the input conditions of the GPU tests ---------------------------------------------------------------------------

@pytest.mark.parametrize('name', sorted(LC.HEAD_CASES))
def test_ohem_cases_tie_exactly_and_only_where_rows_are_duplicates(name):
    """f32 per-ROI losses of rows that are not exact duplicates differ by more than 1e-4 relative, so the rounding differences
    between the host's and the device's f32 cannot reorder them; exact duplicates straddle the K-th place (K < P)."""
    from xdet import losses as L
    cls, reg, labels, targets, fg, k = LC.head_case(name)
    res = L.host_head_loss(cls, reg, labels, targets, fg, k)
    grp = LC.duplicate_groups(cls, reg, labels, targets)
    N, P = labels.shape
    K = res.select.shape[1]
    for n in range(N):
        order = np.lexsort((np.arange(P), -res.per_roi[n]))
        v, g = res.per_roi[n][order].astype(np.float64), grp[n][order]
        differ = g[1:] != g[:-1]
        if (labels[n] >= 0).any():
            rel = (v[:-1] - v[1:]) / np.maximum(np.abs(v[:-1]), 1e-30)
            assert rel[differ].min() > 1e-4, (name, n, rel[differ].min())
            assert (v[:-1][~differ] == v[1:][~differ]).all()
            assert (~differ).sum() >= 3
            if 0 < k < P:
                assert g[K - 1] == g[K] and order[K - 1] < order[K], (name, n)
        else:
            assert not v.any()


def test_logits_to_50_stay_in_the_normal_range():
    """magnitudes up to 50 with row gaps below 80: no softmax term is subnormal, so whether a gradient entry is zero does not
    hinge on how a subnormal rounds"""
    cls = LC.head_case('logits_to_50')[0]
    assert np.abs(cls).max() > 49 and (cls.max(-1) - cls.min(-1)).max() <= 80.


def test_f32_statement_distance_from_float64():
    """prints the figure of this file's docstring: the GPU bar is four times it"""
    worst = max(rpn_distance(n)[0] for n in LC.RPN_CASES)
    worst = max([worst] + [head_distance(n)[0] for n in LC.HEAD_CASES])
    print('f32 NumPy statement vs float64, largest distance / max(1, |value|) = %.3e' % worst)
    assert 0 < worst < 1e-5


def rpn_distance(name):
    from xdet import losses as L
    cls, loc, labels, targets, api, fg, seed = LC.rpn_case(name)
    a = L.host_rpn_loss(LC.anchor_major(cls, 2), LC.anchor_major(loc, 4), labels, targets, api, fg, seed)
    b = L.host_rpn_loss(LC.anchor_major(cls, 2), LC.anchor_major(loc, 4), labels, targets, api, fg, seed, dtype=np.float64)
    return max(LC.distance(x, y) for x, y in ((a.losses, b.losses), (a.grad_cls, b.grad_cls), (a.grad_loc, b.grad_loc))), a, b


def head_distance(name):
    from xdet import losses as L
    args = LC.head_case(name)
    a, b = L.host_head_loss(*args), L.host_head_loss(*args, dtype=np.float64)
    return max(LC.distance(x, y) for x, y in ((a.losses, b.losses), (a.per_roi, b.per_roi), (a.grad_cls, b.grad_cls),
                                              (a.grad_reg, b.grad_reg))), a, b


# ---- argument errors ---------------------------------------------------------------------------------------------------

def bad_calls():
    from xdet import losses as L
    c, b = np.zeros((2, 4, 6), f32), np.zeros((2, 4, 12), f32)
    lab, tg = np.zeros((2, 12), np.int32), np.zeros((2, 12, 4), f32)
    hc, hr, hl, ht = np.zeros((2, 8, 21), f32), np.zeros((2, 8, 4), f32), np.zeros((2, 8), np.int32), np.zeros((2, 8, 4), f32)
    return [
        lambda: L.rpn_loss(c, b, lab, tg, 0, 0.25),                          # anchors_per_image
        lambda: L.rpn_loss(c, b, lab, tg, 20000, 0.25),                      # S > 32768
        lambda: L.rpn_loss(c, b, lab, tg, 4, 0.),                            # fg_ratio
        lambda: L.rpn_loss(c, b, lab, tg, 4, 1.5),
        lambda: L.rpn_loss(c, b, lab, tg, 4, 0.25, sigma=0.),
        lambda: L.rpn_loss(c, b, lab, tg, 4, 0.25, sigma=float('nan')),
        lambda: L.rpn_loss(c, b[:, :3], lab, tg, 4, 0.25),                   # shapes
        lambda: L.rpn_loss(c, b, lab[:, :5], tg, 4, 0.25),
        lambda: L.rpn_loss(c[:0], b[:0], lab[:0], tg[:0], 4, 0.25),
        lambda: L.head_loss(hc, hr, hl, ht, 0., 4),
        lambda: L.head_loss(hc, hr, hl, ht, 0.25, -1),
        lambda: L.head_loss(hc, hr, hl, ht, 0.25, 4, sigma=-1.),
        lambda: L.head_loss(hc[..., :1], hr, hl, ht, 0.25, 4),               # C < 2
        lambda: L.head_loss(np.zeros((2, 8, 200), f32), hr, hl, ht, 0.25, 4),   # C > 128
        lambda: L.head_loss(hc, hr[:, :3], hl, ht, 0.25, 4),
        lambda: L.head_loss(hc, hr, hl[:, :3], ht, 0.25, 4),
    ]


def test_argument_errors_are_raised_before_any_gpu_work(monkeypatch):
    import xdet
    from xdet import runtime

    def no_gpu(*a, **k):
        raise AssertionError('GPU work before the argument checks')
    monkeypatch.setattr(runtime, 'to_device', no_gpu)
    monkeypatch.setattr(runtime, 'DeviceBuffer', no_gpu)
    for call in bad_calls():
        with pytest.raises(xdet.InvalidArgumentError):
            call()


def test_c_abi_rejects_bad_arguments_before_any_gpu_work():
    """XDET_ERR_INVALID_ARG with no device pointer touched (host pointers would fault a launch)"""
    from xdet import _lib
    l = _lib.lib()
    a = np.zeros(4096, f32)
    p = a.ctypes.data
    ok_rpn = dict(ld=8, cls_off=0, box_off=4, N=1, Hh=2, Ww=2, A=1, api=2, fg=0.25, sigma=1.)

    def rpn(**kw):
        v = dict(ok_rpn)
        v.update(kw)
        return l.xdet_rpn_loss(p, v['ld'], v['cls_off'], v['box_off'], v['N'], v['Hh'], v['Ww'], v['A'], p, p, v['api'], v['fg'], 0,
                               v['sigma'], v.get('ws', p), p, p, p, v.get('grad', p), None)
    for kw in (dict(N=0), dict(A=0), dict(ld=6), dict(cls_off=1), dict(box_off=2), dict(box_off=0), dict(box_off=8), dict(api=0),
               dict(api=40000), dict(fg=0.), dict(fg=2.), dict(sigma=0.), dict(ws=None), dict(grad=p + 4), dict(N=1 << 20, Hh=1 << 10)):
        assert rpn(**kw) == -1, kw
    ok_head = dict(ld=28, cls_off=0, reg_off=21, N=2, P=8, C=21, fg=0.25, k=4, sigma=1.)

    def head(**kw):
        v = dict(ok_head)
        v.update(kw)
        return l.xdet_head_loss(p, v['ld'], v['cls_off'], v['reg_off'], v['N'], v['P'], v['C'], p, p, v['fg'], v['k'], v['sigma'],
                                v.get('ws', p), p, p, v.get('select', p), p, None)
    for kw in (dict(N=0), dict(P=0), dict(P=8193), dict(C=1), dict(C=129, ld=160, reg_off=129), dict(ld=24), dict(reg_off=20),
               dict(k=-1), dict(fg=0.), dict(sigma=float('inf')), dict(ws=None), dict(select=None), dict(N=1025)):
        assert head(**kw) == -1, kw
    assert l.xdet_losses_workspace_bytes(128, 256) > 0 and l.xdet_losses_workspace_bytes(129, 256) == 0
    assert l.xdet_losses_workspace_bytes(1024, 0) > 0 and l.xdet_losses_workspace_bytes(1025, 0) == 0
    assert 0 < l.xdet_losses_workspace_bytes(8, 0) <= l.xdet_losses_workspace_bytes(8, 256)
