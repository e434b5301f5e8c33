"""host_batch_norm_forward / host_batch_norm_backward (xdet/train_ops.py), the NumPy statements of xdet_batch_norm_forward /
_backward: in float64 against torch.nn.functional.batch_norm and torch.autograd in both modes, with and without ReLU; the f32
statement's distance from the float64 one on every case of tests/batch_norm_cases.py, which
tests/golden/batch_norm_f32_distance.npz records and the GPU bar is read from; that the bar has teeth (an E[x^2] - E[x]^2
variance in f32 misses it on `offset`, a dx without the xhat dgamma / M term and a mask from a recomputed y miss it too); the
merge of the large-separable block's two branches into one conv pair and the split of its gradients; the argument checks of
the C door and its workspace size against the layout walk of csrc/batchnorm_layout.h."""
import os
import subprocess
import sys

import numpy as np
import pytest

import batch_norm_cases as BC
import conv_backward_cases as CC

f32, f64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _torch_forward(c, training, relu):
    import torch
    import torch.nn.functional as F
    x = torch.tensor(np.asarray(c['x'], f64), requires_grad=True)
    gamma = torch.tensor(np.asarray(c['gamma'], f64), requires_grad=True)
    beta = torch.tensor(np.asarray(c['beta'], f64), requires_grad=True)
    rm, rv = torch.tensor(np.asarray(c['moving_mean'], f64)), torch.tensor(np.asarray(c['moving_var'], f64))
    z = F.batch_norm(x, rm, rv, gamma, beta, training=training, momentum=1 - BC.MOMENTUM, eps=BC.EPS)
    return x, gamma, beta, rm, rv, (torch.relu(z) if relu else z), z


@pytest.mark.parametrize('relu', [False, True])
@pytest.mark.parametrize('training', [True, False])
@pytest.mark.parametrize('name', ['ragged', 'large_sep_widths', 'offset', 'chunk_tail'])
def test_float64_statements_against_torch(name, training, relu):
    """forward: y and the updated running statistics (torch's momentum is 1 - this one; it too updates with the unbiased
    variance); backward: dx, dgamma, dbeta by autograd, the mask taken from the given y"""
    import torch
    from xdet.ops import host_batch_norm_forward, host_batch_norm_backward
    c = BC.make_case(name)
    y, mean, invstd, mm, mv = host_batch_norm_forward(c['x'], c['gamma'], c['beta'], BC.EPS, training, BC.MOMENTUM,
                                                      c['moving_mean'], c['moving_var'], relu, f64)
    tx, tg, tb, rm, rv, ty, tz = _torch_forward(c, training, relu)
    assert y.dtype == f64 and np.abs(y - ty.detach().numpy()).max() <= 1e-11 * max(1., np.abs(y).max())
    assert np.abs(mm - rm.numpy()).max() <= 1e-12 * np.abs(mm).max() and np.abs(mv - rv.numpy()).max() <= 1e-12 * np.abs(mv).max()
    if not training:
        assert np.array_equal(mm, np.asarray(c['moving_mean'], f64)) and np.array_equal(mv, np.asarray(c['moving_var'], f64))
    g = torch.tensor(np.asarray(c['dy'], f64))
    if relu:
        g = g * torch.tensor((y > 0).astype(f64))
    (tz * g).sum().backward()
    dx, dg, db = host_batch_norm_backward(c['x'], y if relu else None, c['dy'], c['gamma'], mean, invstd, training, f64)
    scale = float(np.abs(c['dy']).max()) * float(np.abs(invstd).max()) * 2
    assert np.abs(dx - tx.grad.numpy()).max() <= 1e-11 * scale
    assert np.abs(dg - tg.grad.numpy()).max() <= 1e-11 * scale * len(c['x'])
    assert np.abs(db - tb.grad.numpy()).max() <= 1e-11 * scale * len(c['x'])


@pytest.mark.parametrize('name', sorted(BC.CASES))
def test_relu_cases_have_zeros_and_positives(name):
    from xdet.ops import host_batch_norm_forward
    c = BC.make_case(name)
    if c['relu']:
        for training in (True, False):
            y = host_batch_norm_forward(c['x'], c['gamma'], c['beta'], BC.EPS, training, BC.MOMENTUM, c['moving_mean'],
                                        c['moving_var'], True)[0]
            assert (y == 0).any() and (y > 0).any(), (name, training)


@pytest.mark.parametrize('training', [True, False])
@pytest.mark.parametrize('name', sorted(BC.CASES))
def test_f32_statement_within_the_bar(name, training):
    d = BC.statement_distances(name, training)
    print(name, training, ' '.join('%s %.2e' % kv for kv in sorted(d.items())), 'bar %.2e' % BC.bar())
    assert max(d.values()) <= BC.bar(), d


def _naive_forward(x, gamma, beta, eps, training, momentum, moving_mean, moving_var, relu, dtype):
    """the variance the contract forbids: E[x^2] - E[x]^2"""
    from xdet.ops import host_batch_norm_forward
    x = np.asarray(x, dtype)
    M = dtype(x.shape[0])
    mean = x.sum(axis=0, dtype=dtype) / M
    var = np.maximum((x * x).sum(axis=0, dtype=dtype) / M - mean * mean, dtype(0))
    return host_batch_norm_forward(x, gamma, beta, eps, False, momentum, mean, var, relu, dtype)


def test_the_bar_has_teeth_naive_variance():
    d = BC.statement_distances('offset', True, forward=_naive_forward)
    print('E[x^2] - E[x]^2 in f32 on offset: var distance %.2e, bar %.2e' % (d['var'], BC.bar()))
    assert d['var'] > 100 * BC.bar()


def test_the_bar_has_teeth_dropped_term_and_recomputed_mask():
    from xdet.ops import host_batch_norm_backward

    def dropped(x, y, dy, gamma, mean, invstd, training, dtype):
        dx, dg, db = host_batch_norm_backward(x, y, dy, gamma, mean, invstd, training, dtype)
        xhat = (np.asarray(x, dtype) - mean) * invstd
        return dx + (gamma * invstd) * xhat * (dg / dtype(len(x))), dg, db

    for name in ('ragged', 'large_sep_widths', 'offset', 'chunk_growth'):
        assert BC.statement_distances(name, True, backward=dropped)['dx'] > 10 * BC.bar(), name

    # a mask recomputed from x instead of the forward's y: planted zeros (and NaNs) of y are not seen
    c = BC.make_case('ragged')
    from xdet.ops import host_batch_norm_forward
    y, mean, invstd = host_batch_norm_forward(c['x'], c['gamma'], c['beta'], BC.EPS, True, BC.MOMENTUM, None, None, True)[:3]
    planted = y.copy()
    pos = np.argwhere(y > 0)[:7]
    planted[tuple(pos.T)] = 0
    re_y = np.maximum(((c['x'] - mean) * invstd) * c['gamma'] + c['beta'], 0)
    got = host_batch_norm_backward(c['x'], re_y, c['dy'], c['gamma'], mean, invstd, True)
    d = BC.backward_distances('ragged', True, planted, mean, invstd, got)
    assert max(d.values()) > 10 * BC.bar(), d


def test_one_row_gives_dx_exactly_zero():
    from xdet.ops import host_batch_norm_forward, host_batch_norm_backward
    c = BC.make_case('one_row')
    for dtype in (f32, f64):
        y, mean, invstd, mm, mv = host_batch_norm_forward(c['x'], c['gamma'], c['beta'], BC.EPS, True, BC.MOMENTUM,
                                                          c['moving_mean'], c['moving_var'], False, dtype)
        assert np.array_equal(mean, np.asarray(c['x'][0], dtype)) and np.all(invstd == dtype(1) / np.sqrt(dtype(BC.EPS)))
        assert np.array_equal(y[0], np.asarray(c['beta'], dtype))
        # the max(M - 1, 1) guard: the moving variance moves towards 0, not towards a NaN
        assert np.isfinite(mv).all() and np.all(mv < np.asarray(c['moving_var'], dtype))
        dx, dg, db = host_batch_norm_backward(c['x'], None, c['dy'], c['gamma'], mean, invstd, True, dtype)
        assert dx.dtype == dtype and np.all(dx == 0) and np.all(dg == 0) and np.array_equal(db, np.asarray(c['dy'][0], dtype))


def test_constant_channel_is_finite():
    d = BC.statement_distances('constant_channel', True)
    assert np.isfinite(list(d.values())).all()


def test_mask_rule_zero_and_nan():
    from xdet.ops import host_batch_norm_backward
    rng = np.random.default_rng(5)
    x, dy, y = rng.standard_normal((6, 3)), rng.standard_normal((6, 3)), np.abs(rng.standard_normal((6, 3)))
    y[1, 0], y[4, 2] = np.nan, 0.
    dy_nan = dy.copy()
    dy_nan[1, 0] = np.nan
    dy0 = dy.copy()
    dy0[1, 0] = dy0[4, 2] = 0
    gamma, mean, invstd = np.ones(3), x.mean(axis=0), 1 / np.sqrt(x.var(axis=0) + 1e-5)
    for dtype in (f32, f64):
        got = host_batch_norm_backward(x, y, dy_nan, gamma, mean, invstd, True, dtype)
        want = host_batch_norm_backward(x, None, dy0, gamma, mean, invstd, True, dtype)
        for u, v in zip(got, want):
            assert u.dtype == dtype and np.isfinite(u).all() and np.array_equal(u, v)
        ev = host_batch_norm_backward(x, y, dy_nan, gamma, mean, invstd, False, dtype)[0]
        assert ev[1, 0] == 0 and ev[4, 2] == 0


def test_merged_branches_reproduce_the_per_branch_gradients():
    """the large-separable block as the model runs it in training mode -- one (15,1) conv of both branches' kernels side by
    side, one (1,15) conv of them stacked -- against the unmerged block in float64: z and, split back, every gradient"""
    from xdet.model import merge_large_sep, split_large_sep_grads
    from xdet.ops import host_conv_backward
    rng = np.random.default_rng(11)
    N, H, W, cin, mid, co = 1, 5, 6, 7, 3, 4
    w = {}
    for br in ('Branch_0', 'Branch_1'):
        p = 'large_sep_feature/%s/' % br
        w[p + 'conv2d/kernel'], w[p + 'conv2d/bias'] = rng.standard_normal((15, 1, cin, mid)) / 5, rng.standard_normal(mid)
        w[p + 'conv2d_1/kernel'], w[p + 'conv2d_1/bias'] = rng.standard_normal((1, 15, mid, co)) / 5, rng.standard_normal(co)
    x, dz = rng.standard_normal((N, H, W, cin)), rng.standard_normal((N, H, W, co))
    ka, ba, kb, bb = merge_large_sep(w, dtype=f64)
    assert ka.shape == (15, 1, cin, 2 * mid) and kb.shape == (1, 15, 2 * mid, co) and ba.shape == (2 * mid,) and bb.shape == (co,)
    t = CC.conv_forward64(x, ka, False) + ba
    z = CC.conv_forward64(t, kb, False) + bb
    want_z, want = 0, {}
    for br in ('Branch_0', 'Branch_1'):
        p = 'large_sep_feature/%s/' % br
        tb = CC.conv_forward64(x, w[p + 'conv2d/kernel'], False) + w[p + 'conv2d/bias']
        want_z = want_z + CC.conv_forward64(tb, w[p + 'conv2d_1/kernel'], False) + w[p + 'conv2d_1/bias']
        dt, want[p + 'conv2d_1/kernel'], want[p + 'conv2d_1/bias'] = host_conv_backward(tb, w[p + 'conv2d_1/kernel'], dz, dtype=f64)
        dxb, want[p + 'conv2d/kernel'], want[p + 'conv2d/bias'] = host_conv_backward(x, w[p + 'conv2d/kernel'], dt, dtype=f64)
        want['out'] = want.get('out', 0) + dxb
    assert np.abs(z - want_z).max() <= 1e-12 * np.abs(want_z).max()
    dt, dkb, dbb = host_conv_backward(t, kb, dz, dtype=f64)
    dx, dka, dba = host_conv_backward(x, ka, dt, dtype=f64)
    got = split_large_sep_grads(dka, dba, dkb, dbb, mid)
    assert sorted(got) == sorted(k for k in want if k != 'out')
    for k in got:
        assert got[k].shape == w[k].shape and np.abs(got[k] - want[k]).max() <= 1e-12 * max(1., np.abs(want[k]).max()), k
    assert np.abs(dx - want['out']).max() <= 1e-12 * np.abs(want['out']).max()
    assert np.array_equal(got['large_sep_feature/Branch_0/conv2d_1/bias'], got['large_sep_feature/Branch_1/conv2d_1/bias'])


def test_python_door_refuses_before_any_gpu_work(monkeypatch):
    import xdet
    from xdet import ops, runtime, train_ops

    def no_gpu(*a, **k):
        raise AssertionError('GPU work before the argument checks')
    for mod in (runtime, ops, train_ops):
        monkeypatch.setattr(mod, 'to_device', no_gpu)
        monkeypatch.setattr(mod, 'DeviceBuffer', no_gpu)
    z = lambda *s: np.zeros(s, f32)
    for call in (lambda: xdet.batch_norm_forward(z(4), z(4), z(4), 1e-5),                                 # no rows
                 lambda: xdet.batch_norm_forward(z(0, 4), z(4), z(4), 1e-5),                              # M = 0
                 lambda: xdet.batch_norm_forward(z(2, 4097), z(4097), z(4097), 1e-5),                     # C above 4096
                 lambda: xdet.batch_norm_forward(z(2, 4), z(4), z(4), 1e-5, training=False),              # eval without statistics
                 lambda: xdet.batch_norm_forward(z(2, 4), z(4), z(4), 1e-5, moving_mean=z(4)),            # one of the two
                 lambda: xdet.batch_norm_backward(z(2, 4), None, z(3, 4), z(4), z(4), z(4)),              # dy's rows
                 lambda: xdet.batch_norm_backward(z(2, 4), z(2, 5), z(2, 4), z(4), z(4), z(4))):          # y's channels
        with pytest.raises(xdet.InvalidArgumentError):
            call()


def test_c_door_refuses_before_any_gpu_work():
    """every refusal of include/xdet.h, with pointers that are never dereferenced (the library loads without a GPU)"""
    from xdet._lib import lib
    l = lib()
    p = 4096
    fw = dict(x=p, ld_x=64, M=70, C=50, gamma=p, beta=p, training=1, mm=p, mv=p, relu=1, y=p, ld_y=64, mean=p, inv=p, ws=p)

    def forward(**kw):
        v = dict(fw, **kw)
        return l.xdet_batch_norm_forward(v['x'], v['ld_x'], v['M'], v['C'], v['gamma'], v['beta'], 1e-5, v['training'], 0.997,
                                         v['mm'], v['mv'], v['relu'], v['y'], v['ld_y'], v['mean'], v['inv'], v['ws'], None)
    big_ld = 2 ** 31 // 70 + 1
    for kw in [dict(M=0), dict(M=-1), dict(C=0), dict(C=4097, ld_x=4097, ld_y=4097), dict(M=2 ** 31 // 50 + 1), dict(ld_x=big_ld),
               dict(ld_y=big_ld), dict(ld_x=49), dict(ld_y=49), dict(x=None), dict(gamma=None), dict(beta=None), dict(y=None),
               dict(mean=None), dict(inv=None), dict(ws=None), dict(training=0, mm=None, mv=None), dict(training=0, mm=None),
               dict(training=0, mv=None), dict(mm=None), dict(mv=None)]:
        assert forward(**kw) == -1, kw
        assert b'batch_norm_forward' in l.xdet_last_error()

    bw = dict(x=p, ld_x=64, y=p, ld_y=64, dy=p, ld_dy=64, M=70, C=50, gamma=p, mean=p, inv=p, training=1, dx=p, ld_dx=64, dg=p,
              db=p, ws=p)

    def backward(**kw):
        v = dict(bw, **kw)
        return l.xdet_batch_norm_backward(v['x'], v['ld_x'], v['y'], v['ld_y'], v['dy'], v['ld_dy'], v['M'], v['C'], v['gamma'],
                                          v['mean'], v['inv'], v['training'], v['dx'], v['ld_dx'], v['dg'], v['db'], v['ws'], None)
    for kw in [dict(M=0), dict(C=0), dict(C=-4), dict(C=4097, ld_x=4097, ld_y=4097, ld_dy=4097, ld_dx=4097),
               dict(M=2 ** 31 // 50 + 1), dict(ld_x=big_ld), dict(ld_y=big_ld), dict(ld_dy=big_ld), dict(ld_dx=big_ld), dict(ld_x=49),
               dict(ld_y=49), dict(ld_dy=49), dict(ld_dx=49), dict(x=None), dict(dy=None), dict(gamma=None), dict(mean=None),
               dict(inv=None), dict(dg=None), dict(db=None), dict(ws=None)]:
        assert backward(**kw) == -1, kw
        assert b'batch_norm_backward' in l.xdet_last_error()
    size = l.xdet_batch_norm_workspace_bytes
    assert size(70, 50) > 0 and size(1, 1) > 0 and size(7200, 490) > 0 and size(2 ** 31 // 4096 - 1, 4096) > 0
    for args in ((0, 50), (70, 0), (70, 4097), (-1, 5), (2 ** 31 // 50 + 1, 50)):
        assert size(*args) == 0, args


SIZES = [(1, 8), (70, 50), (129, 4), (65537, 5), (7200, 490), (3, 4096), (65536, 1), (1048577, 3)]


def test_workspace_size_is_the_layout_walk(tmp_path):
    """a stand-alone host program walks bn_layout (csrc/batchnorm_layout.h) with a measuring and a carving WsWalk; the
    library's size entry point returns the same bytes, and the chunk rule is max(64, ceil(M / 1024)) rows"""
    from xdet._lib import lib
    src = tmp_path / 'bn_layout_check.cpp'
    src.write_text('#include "batchnorm_layout.h"\n#include <cstdio>\n#include <cstdlib>\n#include <vector>\n'
                   'using namespace xdet;\n'
                   'int main(int argc, char** argv) {\n'
                   '  for (int i = 1; i + 1 < argc; i += 2) {\n'
                   '    const int M = atoi(argv[i]), C = atoi(argv[i + 1]);\n'
                   '    const BnSums p = bn_sums(M);\n'
                   '    const size_t n = ws_measure(4, bn_layout, p, C);\n'
                   '    std::vector<unsigned char> block(n);\n'
                   '    const BnWorkspace w = ws_carve(block.data(), 4, bn_layout, p, C);\n'
                   '    const bool ok = (unsigned char*)w.first == block.data() && w.second == w.first + (size_t)p.n_chunks * C &&\n'
                   '                    (unsigned char*)(w.second + (size_t)p.n_chunks * C) == block.data() + n;\n'
                   '    printf("%d %d %d %zu %d\\n", M, p.rows_per_chunk, p.n_chunks, n, ok ? 1 : 0);\n'
                   '  }\n'
                   '  return 0;\n'
                   '}\n')
    exe = str(tmp_path / 'bn_layout_check')
    subprocess.check_call([os.environ.get('CXX', 'c++'), '-std=c++17', '-O1', '-Wall', '-Werror', '-fsanitize=address,undefined',
                           '-fno-sanitize-recover=all', '-I', os.path.join(ROOT, 'x-detector_amd', 'csrc'), str(src), '-o', exe])
    r = subprocess.run([exe] + [str(v) for mc in SIZES for v in mc], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 0, r.stderr.decode()
    rows = [tuple(int(v) for v in line.split()) for line in r.stdout.decode().splitlines()]
    assert len(rows) == len(SIZES)
    for (M, C), (m, per, chunks, nbytes, ok) in zip(SIZES, rows):
        want_per = max(64, -(-M // 1024))
        assert (m, per, chunks, ok) == (M, want_per, -(-M // want_per), 1), (M, C)
        assert chunks <= 1024 and nbytes == 2 * chunks * C * 4
        assert lib().xdet_batch_norm_workspace_bytes(M, C) == nbytes, (M, C)


def test_new_symbols_are_exported():
    import re
    from xdet import _lib
    out = subprocess.check_output(['nm', '-D', '--defined-only', _lib.LIB_PATH]).decode()
    exported = set(re.findall(r'\sT\s+(xdet_[a-z0-9_]+)', out))
    assert {'xdet_batch_norm_forward', 'xdet_batch_norm_backward', 'xdet_batch_norm_workspace_bytes'} <= exported
    assert _lib.lib().xdet_batch_norm_workspace_bytes.restype is _lib.c_size_t


def test_f32_statement_distance_is_the_recorded_one():
    """numpy builds may order their sums differently: the recorded figure must be of the size measured here (within 2x either
    way), so the GPU bar read from the file is the bar this module would compute"""
    d = BC.f32_statement_distance()
    rec = float(np.load(BC.GOLDEN)['f32_distance'])
    print('f32 statement vs float64: measured %.3e, recorded %.3e -> GPU bar %.3e (floor %.3e)' % (d, rec, BC.bar(), BC.FLOOR))
    assert 0 < d and rec / 2 <= d <= rec * 2, (d, rec)
    assert BC.bar() == max(4 * rec, BC.FLOOR)
    assert sorted(np.load(BC.GOLDEN)['cases'].tolist()) == sorted(BC.CASES)


if __name__ == '__main__' and '--write' in sys.argv:
    sys.path.insert(0, os.path.join(ROOT, 'x-detector_amd'))
    d = BC.f32_statement_distance()
    np.savez(BC.GOLDEN, f32_distance=np.float64(d), cases=np.array(sorted(BC.CASES)))
    print('wrote %s: %.3e' % (BC.GOLDEN, d))
