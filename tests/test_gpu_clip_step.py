"""The clipped momentum step on the GPU, op level (xdet_momentum_step_clipped, csrc/optimizer.hip): xdet_grad_stats, then the
clipped step on its record, against the NumPy statements -- host_grad_sq (the record's f32 sum in the device's order; the
float64 host_grad_stats bounds it), host_clip_scale and host_momentum_step(..., scale=) -- for equal bits of var, accum and
the scale, and of l2 against the unclipped step's (l2 reads the values before the update and no gradient).

The table: slots of 1, 5, 4095, 4096, 4097 and 9000 elements (chunk ends and short last chunks) and one more whose grad alone
lies 4 bytes off a 16-byte boundary (the scalar path), decay mixed.  One packed array per role; behind every slot lie GAP
elements that are nobody's: NaN in the gradient array, a canary in var and accum."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
CHUNK, GAP = 4096, 8
CANARY = f32(-1234.5)
U = 2.0 ** -24
LR, M, WD = 0.1, 0.9, 2e-4
ONE = 0x3f800000

# (n, decay, grad's offset from the 16-byte boundary in floats)
TABLE = [(1, True, 0), (5, False, 0), (4095, True, 0), (4096, False, 0), (4097, True, 0), (9000, False, 0), (4099, True, 1)]
EXACT = [(2, True, 0)]                                   # grad [3, 4]: a norm of exactly 5


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def make_table(spec, seed, grad=None):
    rng = np.random.default_rng(seed)
    offs, goffs, at = [], [], 0
    for n, _, shift in spec:
        at = -(-at // 4) * 4
        offs.append(at)
        goffs.append(at + shift)
        at += n + GAP
    total = at
    t = {'spec': spec, 'offs': offs, 'goffs': goffs, 'total': total,
         'var': np.full(total, CANARY, f32), 'accum': np.full(total, CANARY, f32), 'grad': np.full(total, np.nan, f32)}
    for i, (o, go, (n, _, _)) in enumerate(zip(offs, goffs, spec)):
        t['var'][o:o + n] = rng.standard_normal(n) * 0.1
        t['accum'][o:o + n] = rng.standard_normal(n) * 0.02
        t['grad'][go:go + n] = rng.standard_normal(n) * 0.01 if grad is None else grad[i]
    return t


def slot_grads(t, grad=None):
    g = t['grad'] if grad is None else grad
    return [g[go:go + n] for go, (n, _, _) in zip(t['goffs'], t['spec'])]


def upload(t, grad=None):
    from xdet.runtime import DeviceTensor, to_device
    var, g, accum = to_device(t['var']), to_device(t['grad'] if grad is None else grad), to_device(t['accum'])
    view = lambda b, o, n: DeviceTensor(b.ptr + 4 * o, (n,), n, owner=b)
    slots = [(view(var, o, n), view(g, go, n), view(accum, o, n), n, d) for o, go, (n, d, _) in zip(t['offs'], t['goffs'], t['spec'])]
    for (v, gg, a, n, d), (_, _, shift) in zip(slots, t['spec']):
        assert v.ptr % 16 == 0 and a.ptr % 16 == 0 and gg.ptr % 16 == 4 * shift
    return slots, (var, g, accum)


def run(t, clip_norm, guard, grad=None, clipped=True):
    """grad_stats and the clipped step (clipped=False: xdet_momentum_step) on a fresh upload
    -> {var, grad, accum as the device holds them afterwards, l2, scale, the record}"""
    from xdet import grad_stats_device, momentum_step_device, train_ops
    from xdet.runtime import DeviceBuffer, synchronize, to_host
    slots, bufs = upload(t, grad)
    rec = grad_stats_device(slots)
    scale = DeviceBuffer(16)
    if clipped:
        l2 = momentum_step_device(slots, LR, M, WD, l2=True, clip=(rec, clip_norm), scale_out=scale, **({'skip': rec} if guard else {}))
    else:
        l2 = momentum_step_device(slots, LR, M, WD, l2=True)
    synchronize()
    out = dict(zip(('var', 'grad', 'accum'), (to_host(b.ptr, (t['total'],)) for b in bufs)))
    out['l2'], out['scale'] = to_host(l2.ptr, (1,))[0], to_host(scale.ptr, (1,))[0] if clipped else None
    out['rec'] = to_host(rec.ptr, (1,), train_ops.GRAD_STATS_DTYPE)[0]
    return out


def statement(t, clip_norm):
    """the NumPy statement of the clipped step -> (var, accum as packed arrays, canaries included, the scale, grad_sq)"""
    from xdet import host_clip_scale, host_grad_sq, host_momentum_step
    sq = host_grad_sq(slot_grads(t))
    scale = host_clip_scale(sq, clip_norm)
    hv, ha = t['var'].copy(), t['accum'].copy()
    for o, go, (n, d, _) in zip(t['offs'], t['goffs'], t['spec']):
        hv[o:o + n], ha[o:o + n] = host_momentum_step(t['var'][o:o + n], t['grad'][go:go + n], t['accum'][o:o + n], LR, M, WD, d, scale=scale)
    return hv, ha, scale, sq


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def check_against_statement(t, got, clip_norm):
    from xdet import host_grad_stats
    hv, ha, scale, sq = statement(t, clip_norm)
    want64 = host_grad_stats(slot_grads(t))[0]
    chunks = sum(-(-n // CHUNK) for n, _, _ in t['spec'])
    k = 1 + 2 + 2 + 8 + max(1, math.ceil(math.log2(chunks)))
    print('clip %g: grad_sq %.9g (float64 %.9g), norm %.9g, scale %.9g' % (clip_norm, got['rec']['grad_sq'], want64, np.sqrt(sq), got['scale']))
    assert bits(got['rec']['grad_sq'])[0] == bits(sq)[0] and abs(float(sq) - want64) <= k * U / (1 - k * U) * want64
    assert int(got['rec']['nonfinite']) == 0                                     # the NaN behind every slot is absent
    assert bits(got['scale'])[0] == bits(scale)[0], (got['scale'], scale)
    assert same(got['var'], hv) and same(got['accum'], ha) and same(got['grad'], t['grad'])
    return scale


@pytest.fixture(scope='module')
def table():
    t = make_table(TABLE, 21)
    t['plain'] = run(t, None, 0, clipped=False)
    t['norm'] = float(np.sqrt(f64(t['plain']['rec']['grad_sq'])))
    return t


def test_the_table_covers_both_access_paths(table):
    sizes = [n for n, _, _ in TABLE]
    assert sizes[:6] == [1, 5, 4095, 4096, 4097, 9000] and [s for _, _, s in TABLE].count(1) == 1
    assert {d for _, d, _ in TABLE} == {True, False} and 0.5 < table['norm'] < 5


@pytest.mark.parametrize('guard', [0, 1])
def test_a_clip_above_the_norm_is_the_unclipped_step(table, guard):
    clip = 2 * table['norm']
    got = run(table, clip, guard)
    assert check_against_statement(table, got, clip) == 1 and bits(got['scale'])[0] == ONE
    p = table['plain']
    assert same(got['var'], p['var']) and same(got['accum'], p['accum']) and bits(got['l2'])[0] == bits(p['l2'])[0]
    assert not same(p['var'], table['var'])


@pytest.mark.parametrize('guard', [0, 1])
@pytest.mark.parametrize('fraction', [0.5, 0.013])
def test_a_clip_below_the_norm_scales_every_gradient(table, guard, fraction):
    clip = fraction * table['norm']
    got = run(table, clip, guard)
    scale = check_against_statement(table, got, clip)
    assert 0 < scale < 1 and abs(float(scale) - fraction) < 1e-5
    p = table['plain']
    assert bits(got['l2'])[0] == bits(p['l2'])[0]                             # l2 reads no gradient
    assert not same(got['var'], p['var']) and not same(got['accum'], p['accum'])
    own = got['var'] != CANARY
    assert own.sum() == sum(n for n, _, _ in TABLE) and (got['accum'][~own] == CANARY).all()


def test_a_norm_equal_to_the_clip_gives_one():
    t = make_table(EXACT, 22, grad=[np.array([3, 4], f32)])
    got, plain = run(t, 5.0, 1), run(t, None, 0, clipped=False)
    assert got['rec']['grad_sq'] == 25 and bits(got['scale'])[0] == ONE
    assert check_against_statement(t, got, 5.0) == 1
    assert same(got['var'], plain['var']) and same(got['accum'], plain['accum']) and bits(got['l2'])[0] == bits(plain['l2'])[0]
    below = run(t, 4.0, 0)                                                      # and a clip of 4 scales by 0.8
    assert check_against_statement(t, below, 4.0) == f32(4) / f32(5)


@pytest.mark.parametrize('slot,element', [(5, 8999), (6, 0), (0, 0)])
def test_one_nan_under_the_guard_stores_nothing(table, slot, element):
    t = table
    grad = t['grad'].copy()
    grad[t['goffs'][slot] + element] = np.nan
    got = run(t, 0.5 * t['norm'], 1, grad=grad)
    assert int(got['rec']['nonfinite']) == 1 and int(got['rec']['first_bad_slot']) == slot and np.isnan(got['rec']['grad_sq'])
    # every byte of var and accum, the memory behind each slot included, is the upload's; l2 is the unguarded value
    assert same(got['var'], t['var']) and same(got['accum'], t['accum']) and same(got['grad'], grad)
    assert bits(got['l2'])[0] == bits(t['plain']['l2'])[0]
    assert np.isnan(got['scale'])                                               # the statement's: the maximum keeps a NaN norm


def test_a_nan_without_the_guard_reaches_every_weight(table):
    """the documented choice of guard = 0: a NaN grad_sq is a NaN scale"""
    t = table
    grad = t['grad'].copy()
    grad[t['goffs'][2] + 7] = np.nan
    got = run(t, 0.5 * t['norm'], 0, grad=grad)
    own = t['var'] != CANARY
    assert np.isnan(got['var'][own]).all() and np.isnan(got['accum'][own]).all()
    assert (got['var'][~own] == CANARY).all() and (got['accum'][~own] == CANARY).all()
    assert bits(got['l2'])[0] == bits(t['plain']['l2'])[0]


def test_the_same_call_gives_the_same_bits(table):
    clip = 0.3 * table['norm']
    a, b = run(table, clip, 1), run(table, clip, 1)
    for k in ('var', 'accum', 'grad'):
        assert same(a[k], b[k]), k
    assert bits(a['l2'])[0] == bits(b['l2'])[0] and bits(a['scale'])[0] == bits(b['scale'])[0]
    assert a['rec'].tobytes() == b['rec'].tobytes()


def test_refusals_by_their_message():
    """the C door's, ahead of any launch (var and accum keep their bytes), and the Python door's"""
    import xdet
    from xdet import grad_stats_device, momentum_step_device
    from xdet._lib import lib, MomentumSlot
    from xdet.runtime import DeviceBuffer, synchronize, to_host
    t = make_table([(5, True, 0)], 23)
    slots, bufs = upload(t)
    rec = grad_stats_device(slots)
    ws = DeviceBuffer(1 << 12)
    tab = (MomentumSlot * 1)(MomentumSlot(slots[0][0].ptr, slots[0][1].ptr, slots[0][2].ptr, 5, 1))

    def refused(table=tab, n=1, stats=rec.ptr, clip=1.0, scale=None, workspace=ws.ptr):
        assert lib().xdet_momentum_step_clipped(table, n, LR, M, WD, None, stats, clip, 1, scale, workspace, None) == -1
        return lib().xdet_last_error().decode()
    for clip in (float('nan'), float('inf'), -float('inf'), 0.0, -1.0):
        assert 'momentum_step_clipped: clip_norm must be finite and positive' in refused(clip=clip)
    assert 'momentum_step_clipped: stats_dev is NULL' in refused(stats=None)
    assert 'momentum_step_clipped: stats_dev must be 4-byte aligned' in refused(stats=rec.ptr + 2)
    assert 'momentum_step_clipped: scale_out must be 4-byte aligned' in refused(scale=rec.ptr + 2)
    # everything xdet_momentum_step refuses
    assert 'momentum_step: an empty slot table' in refused(n=0)
    assert 'momentum_step: an empty slot table' in refused(table=None)
    assert 'momentum_step: workspace is NULL' in refused(workspace=None)
    b = slots[0][0].ptr
    assert 'a slot with a NULL var, grad or accum' in refused(table=(MomentumSlot * 1)(MomentumSlot(b, None, b, 5, 1)))
    assert 'a slot with n <= 0' in refused(table=(MomentumSlot * 1)(MomentumSlot(b, b, b, 0, 1)))
    # the Python door
    for kw, msg in ((dict(clip=(rec, float('nan'))), 'clip_norm must be finite and positive'),
                    (dict(clip=(rec, 0)), 'clip_norm must be finite and positive'),
                    (dict(clip=(None, 1.0)), 'momentum_step: clip must be'),
                    (dict(clip=(rec, 1.0), skip=DeviceBuffer(16)), 'skip must be the same record'),
                    (dict(scale_out=DeviceBuffer(16)), 'scale_out goes with clip='),
                    (dict(clip=(rec, 1.0), scale_out=np.zeros(1, f32)), 'scale_out goes with clip=')):
        with pytest.raises(xdet.InvalidArgumentError) as e:
            momentum_step_device(slots, LR, M, WD, **kw)
        assert msg in str(e.value), (kw, str(e.value))
    synchronize()
    assert same(to_host(bufs[0].ptr, (t['total'],)), t['var']) and same(to_host(bufs[2].ptr, (t['total'],)), t['accum'])
