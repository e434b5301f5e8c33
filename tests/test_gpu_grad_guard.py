"""The guard of the optimizer step on the GPU, op level (csrc/optimizer.hip): xdet_grad_stats against the NumPy statement
(host_grad_stats) and xdet_momentum_step_guarded against xdet_momentum_step, over slot tables on either side of the vector
and the chunk, a slot on the scalar path, and one slot of more than 1024 chunks (the fold loops).

One packed array per role; behind every slot lie GAP elements that are nobody's: NaN in the gradient array -- an element
past a slot's end is absent, so a table of finite gradients must count none of them -- and a canary in var and accum, which
every step must leave alone."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
CHUNK = 4096                                             # xdet_momentum_step's chunk (include/xdet.h)
GAP = 8
CANARY = f32(-1234.5)
U = 2.0 ** -24
LR, M, WD = 0.1, 0.9, 2e-4

# (n, decay, aligned): sizes on either side of the vector and the chunk, decay on and off; slot 6's three pointers are 4 bytes
# off a 16-byte boundary, so it takes the scalar path throughout
SMALL = [(1, True, True), (3, False, True), (4095, True, True), (4096, False, True), (4097, True, True), (2 * 4096 + 5, False, True),
         (4099, True, False), (6, False, True)]
BIG = [(1025 * CHUNK, True, True)]

# where one non-finite element goes -> [(slot, element)], and what the record must say
PLACES = {
    'the last element of a short last chunk': [(4, 4096)],
    'the scalar tail of a vectorised slot': [(5, 2 * 4096 + 4)],
    'element 0 of the last slot': [(7, 0)],
    'a slot without decay': [(3, 100)],
    'two slots at once': [(6, 4098), (2, 4094)],
}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def make_table(spec, seed):
    rng = np.random.default_rng(seed)
    offs, at = [], 0
    for n, _, aligned in spec:
        at = -(-at // 4) * 4 + (0 if aligned else 1)
        offs.append(at)
        at += n + GAP
    total = at
    var = (rng.standard_normal(total) * 0.1).astype(f32)
    grad = (rng.standard_normal(total) * 0.01).astype(f32)
    accum = (rng.standard_normal(total) * 0.02).astype(f32)
    own = np.zeros(total, bool)
    for o, (n, _, _) in zip(offs, spec):
        own[o:o + n] = True
    var[~own], accum[~own], grad[~own] = CANARY, CANARY, np.nan
    return {'spec': spec, 'offs': offs, 'total': total, 'var': var, 'grad': grad, 'accum': accum, 'own': own}


def upload(t, grad=None):
    from xdet.runtime import DeviceTensor, to_device
    var, g, accum = to_device(t['var']), to_device(t['grad'] if grad is None else grad), to_device(t['accum'])
    view = lambda b, o, n: DeviceTensor(b.ptr + 4 * o, (n,), n, owner=b)
    slots = [(view(var, o, n), view(g, o, n), view(accum, o, n), n, d) for o, (n, d, _) in zip(t['offs'], t['spec'])]
    for (v, gg, a, n, d), (_, _, aligned) in zip(slots, t['spec']):
        assert all((x.ptr % 16 == 0) == aligned and x.ptr % 4 == 0 for x in (v, gg, a))
    return slots, (var, g, accum)


def download(t, bufs):
    from xdet.runtime import synchronize, to_host
    synchronize()
    return tuple(to_host(b.ptr, (t['total'],)) for b in bufs)


def record(rec):
    from xdet import train_ops
    from xdet.runtime import synchronize, to_host
    synchronize()
    r = to_host(rec.ptr, (1,), train_ops.GRAD_STATS_DTYPE)[0]
    return r['grad_sq'], int(r['nonfinite']), int(r['first_bad_slot']), int(r['zero'])


def l2_value(l2):
    from xdet.runtime import synchronize, to_host
    synchronize()
    return to_host(l2.ptr, (1,))


def plain_step(t):
    """xdet_momentum_step on a fresh upload -> (var, grad, accum as the device holds them afterwards, l2)"""
    from xdet import momentum_step_device
    slots, bufs = upload(t)
    l2 = momentum_step_device(slots, LR, M, WD, l2=True)
    return download(t, bufs) + (l2_value(l2),)


@pytest.fixture(scope='module')
def small():
    t = make_table(SMALL, 11)
    t['plain'] = plain_step(t)
    return t


@pytest.fixture(scope='module')
def big():
    t = make_table(BIG, 12)
    t['plain'] = plain_step(t)
    return t


def grad_sq_bound(t):
    """the order of include/xdet.h: a term is squared (1 rounding) and passes 2 levels inside its vector, 2 over the thread's
    vectors, 8 over the chunk's threads and ceil(log2(chunks)) over the chunk partials; all terms are non-negative, so the
    relative error is at most gamma_k -- and the bar tests/test_gpu_train_step.py applies to l2 is 64 * 2^-24"""
    chunks = sum(-(-n // CHUNK) for n, _, _ in t['spec'])
    k = 1 + 2 + 2 + 8 + math.ceil(math.log2(chunks))
    assert k * U / (1 - k * U) <= 64 * U, (k, chunks)
    return 64 * U, chunks


def check_finite_table(t):
    from xdet import grad_stats_device, host_grad_stats, momentum_step_device
    got = []
    for _ in range(2):
        slots, bufs = upload(t)
        got.append(record(grad_stats_device(slots)))
        assert np.array_equal(bits(download(t, bufs)[1]), bits(t['grad']))          # (it reads only, grad included)
    assert bits(got[0][0]) == bits(got[1][0]) and got[0][1:] == got[1][1:]          # the same bits on every run
    sq, bad, first, zero = got[0]
    want, wbad, wfirst = host_grad_stats([t['grad'][o:o + n] for o, (n, _, _) in zip(t['offs'], t['spec'])])
    bound, chunks = grad_sq_bound(t)
    err = abs(float(sq) - want) / want
    print('grad_sq = %.9g, float64 %.9g: relative error %.3g, bar %.3g (%d chunks)' % (sq, want, err, bound, chunks))
    assert (bad, first, zero) == (0, -1, 0) and (wbad, wfirst) == (0, -1)           # the NaN behind every slot is absent
    assert want > 0 and err <= bound, (err, bound)
    # the guarded step on a record that says go: xdet_momentum_step bit for bit, var, accum (the canaries with them) and l2
    slots, bufs = upload(t)
    rec = grad_stats_device(slots)
    l2 = momentum_step_device(slots, LR, M, WD, l2=True, skip=rec)
    v, g, a = download(t, bufs)
    pv, pg, pa, pl2 = t['plain']
    assert np.array_equal(bits(v), bits(pv)) and np.array_equal(bits(a), bits(pa)) and np.array_equal(bits(g), bits(pg))
    assert bits(l2_value(l2))[0] == bits(pl2)[0]
    assert not np.array_equal(bits(pv), bits(t['var'])) and (pv[~t['own']] == CANARY).all() and (pa[~t['own']] == CANARY).all()


def check_poisoned_table(t, places, poison):
    """-> nothing; the record counts and names, the guarded step stores nothing and still writes l2"""
    from xdet import grad_stats_device, host_grad_stats, momentum_step_device
    grad = t['grad'].copy()
    for slot, el in places:
        assert 0 <= el < t['spec'][slot][0]
        grad[t['offs'][slot] + el] = poison
    slots, bufs = upload(t, grad)
    rec = grad_stats_device(slots)
    l2 = momentum_step_device(slots, LR, M, WD, l2=True, skip=rec)
    sq, bad, first, zero = record(rec)
    _, wbad, wfirst = host_grad_stats([grad[o:o + n] for o, (n, _, _) in zip(t['offs'], t['spec'])])
    assert (wbad, wfirst) == (len(places), min(s for s, _ in places))
    assert (bad, first, zero) == (wbad, wfirst, 0) and not np.isfinite(sq), (sq, bad, first, zero)
    v, g, a = download(t, bufs)
    # every byte of var and accum, the memory behind each slot included, is the upload's
    assert np.array_equal(bits(v), bits(t['var'])) and np.array_equal(bits(a), bits(t['accum']))
    assert np.array_equal(bits(g), bits(grad))
    assert bits(l2_value(l2))[0] == bits(t['plain'][3])[0]                          # l2 is defined either way: the unguarded value


def test_finite_gradients_small_table(small):
    check_finite_table(small)


def test_plain_step_is_still_the_host_statement(small):
    """xdet_momentum_step is now the guarded call with skip_dev = NULL: still host_momentum_step bit for bit"""
    from xdet import host_momentum_step
    t = small
    hv, ha = t['var'].copy(), t['accum'].copy()
    for o, (n, d, _) in zip(t['offs'], t['spec']):
        hv[o:o + n], ha[o:o + n] = host_momentum_step(t['var'][o:o + n], t['grad'][o:o + n], t['accum'][o:o + n], LR, M, WD, d)
    pv, pg, pa, pl2 = t['plain']
    assert np.array_equal(bits(pv), bits(hv)) and np.array_equal(bits(pa), bits(ha))
    want = sum(float((t['var'][o:o + n].astype(f64) ** 2).sum()) for o, (n, d, _) in zip(t['offs'], t['spec']) if d) / 2
    assert abs(float(pl2[0]) - want) / want <= 64 * U


@pytest.mark.parametrize('poison', [np.nan, np.inf, -np.inf], ids=['nan', '+inf', '-inf'])
@pytest.mark.parametrize('place', sorted(PLACES))
def test_one_non_finite_element_holds_the_step(small, place, poison):
    check_poisoned_table(small, PLACES[place], f32(poison))


def test_absent_elements_are_never_counted(small):
    """poison past n: the gaps hold NaN already (checked by the finite test); here +inf and -inf as well, and a poisoned
    element inside the table is still counted once"""
    from xdet import grad_stats_device
    t = small
    grad = t['grad'].copy()
    gaps = np.flatnonzero(~t['own'])
    grad[gaps[0::3]], grad[gaps[1::3]] = np.inf, -np.inf
    slots, _ = upload(t, grad)
    assert record(grad_stats_device(slots))[1:] == (0, -1, 0)
    grad[t['offs'][0]] = np.inf                            # the one element of slot 0, NaN right behind it
    slots, _ = upload(t, grad)
    assert record(grad_stats_device(slots))[1:] == (1, 0, 0)


def test_more_than_1024_chunks(big):
    """one slot of 1025 chunks: the one-workgroup fold loops over its partials"""
    check_finite_table(big)
    n = BIG[0][0]
    check_poisoned_table(big, [(0, n - 1)], f32(np.nan))
    check_poisoned_table(big, [(0, 1024 * CHUNK), (0, 5)], f32(-np.inf))     # the last chunk, past the fold's first 1024, and the first
