"""The one table per language that states how the checkpoint's tensors sit inside the merged tensors of the RPN head, the head
and the large-separable block: csrc/merged_layers.h, checked by a stand-alone host program (tests/merged_layers_check.cpp: its
own main, nothing loaded into Python) built with the host compiler under AddressSanitizer and UndefinedBehaviorSanitizer, and
xdet.train.merged_layout, checked against np.concatenate.  The tests' own statement of the layout is weight_pack_cases.py and
the concatenations written out below; neither is derived from the tables.  No device."""
import os
import subprocess

import numpy as np
import pytest

import weight_pack_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'x-detector_amd', 'csrc')

f32 = np.float32
# head 21|4 at K = 7; RPN 44|88 at hid = 5; large-separable cin = 3, mid = 2, co = 5
SIZES = {'final_head': dict(nc=21, co=3, fcw=7), 'rpn_head': dict(A=22, cin=2, hid=5), 'large_sep_feature': dict(cin=3, mid=2, co=5)}


def test_header_merges_what_it_describes_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / 'merged_layers_check')
    cxx = os.environ.get('CXX', 'c++')
    subprocess.check_call([cxx, '-std=c++17', '-O1', '-g', '-Wall', '-Werror', '-fsanitize=address,undefined',
                           '-fno-sanitize-recover=all', '-I', CSRC, os.path.join(ROOT, 'tests', 'merged_layers_check.cpp'),
                           '-o', exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    out, err = r.stdout.decode(), r.stderr.decode()
    assert r.returncode == 0, (out, err)
    assert 'runtime error' not in err and 'AddressSanitizer' not in err, err
    assert out.startswith('ok: '), out


def _tensors(group):
    """every variable of a group in its checkpoint shape, all of distinct bit patterns (NaN payloads and -0 among them)"""
    from xdet.train import merged_shapes
    shapes = merged_shapes(group, **SIZES[group])
    flat = C.patterns(sum(int(np.prod(s)) for s in shapes.values()), seed=7)
    out, at = {}, 0
    for name, shape in shapes.items():
        n = int(np.prod(shape))
        out[name], at = flat[at:at + n].reshape(shape).copy(), at + n
    return out


def _concatenate(group, t):
    """the merged tensors of a group in np.concatenate's words, {key: [outer, W] array}"""
    if group == 'large_sep_feature':
        b0, b1 = 'large_sep_feature/Branch_0/', 'large_sep_feature/Branch_1/'
        return {'K_a': np.concatenate([t[b0 + 'conv2d/kernel'], t[b1 + 'conv2d/kernel']], axis=3).reshape(15 * 3, 4),
                'b_a': np.concatenate([t[b0 + 'conv2d/bias'], t[b1 + 'conv2d/bias']]).reshape(1, 4),
                'K_b': np.concatenate([t[b0 + 'conv2d_1/kernel'], t[b1 + 'conv2d_1/kernel']], axis=2).reshape(15, 20)}
    if group == 'rpn_head':
        p = 'rpn_head/'
        return {'K_0': t[p + 'conv2d/kernel'].reshape(9 * 2, 5), 'b_0': t[p + 'conv2d/bias'].reshape(1, 5),
                'K_1': np.concatenate([t[p + 'conv2d_1/kernel'].reshape(-1, 44), t[p + 'conv2d_2/kernel'].reshape(-1, 88)], axis=1),
                'b_1': np.concatenate([t[p + 'conv2d_1/bias'], t[p + 'conv2d_2/bias']]).reshape(1, 132)}
    p = 'final_head/'
    return {'K_0': t[p + 'subnet_fc/kernel'], 'b_0': t[p + 'subnet_fc/bias'].reshape(1, 7),
            'K_1': np.concatenate([t[p + 'fc_cls/kernel'], t[p + 'fc_loc/kernel']], axis=1),
            'b_1': np.concatenate([t[p + 'fc_cls/bias'], t[p + 'fc_loc/bias']]).reshape(1, 25)}


@pytest.mark.parametrize('group', sorted(SIZES))
def test_layout_is_the_concatenation_and_split_undoes_it(group):
    from xdet import host_concat, host_split
    from xdet.train import merged_layout, merged_shapes
    layout, shapes, t = merged_layout(group, **SIZES[group]), merged_shapes(group, **SIZES[group]), _tensors(group)
    want = _concatenate(group, t)
    assert [key for key, _, _ in layout] == list(want)
    for key, outer, parts in layout:
        assert 1 <= len(parts) <= 2 and all(w * outer == int(np.prod(shapes[n])) for n, w in parts), key
        merged = host_concat([t[n] for n, _ in parts], outer)
        assert merged.shape == want[key].shape and np.array_equal(C.bits(merged), C.bits(want[key])), key
        back = host_split(merged, outer, [w for _, w in parts])
        for (n, _), b in zip(parts, back):
            assert np.array_equal(C.bits(b.reshape(shapes[n])), C.bits(t[n])), n


def test_the_tables_name_every_variable_once():
    from xdet import train
    names = {}
    for group in SIZES:
        names[group] = [n for _, _, parts in train.merged_layout(group, **SIZES[group]) for n, _ in parts]
        assert list(train.merged_shapes(group, **SIZES[group])) == list({'large_sep_feature': train.LARGE_SEP_VARIABLES[:8],
                                                                        'rpn_head': train.RPN_HEAD_VARIABLES,
                                                                        'final_head': train.HEAD_VARIABLES}[group])
    key, addends = train.LARGE_SEP_BIAS_SUM                    # the one relation that is no concatenation: b_b = b0 + b1
    assert key == 'b_b' and addends == ('large_sep_feature/Branch_0/conv2d_1/bias', 'large_sep_feature/Branch_1/conv2d_1/bias')
    names['large_sep_feature'] += list(addends)
    for group, want in (('large_sep_feature', train.LARGE_SEP_VARIABLES[:8]), ('rpn_head', train.RPN_HEAD_VARIABLES),
                        ('final_head', train.HEAD_VARIABLES)):
        assert sorted(names[group]) == sorted(want) and len(set(names[group])) == len(want), group


def test_merge_large_sep_and_its_adjoint_follow_the_table():
    from xdet.train import merge_large_sep, split_large_sep_grads, LARGE_SEP_BIAS_SUM
    t = _tensors('large_sep_feature')
    want = _concatenate('large_sep_feature', t)
    ka, ba, kb, bb = merge_large_sep(t)
    assert ka.shape == (15, 1, 3, 4) and ba.shape == (4,) and kb.shape == (1, 15, 4, 5) and bb.shape == (5,)
    for got, key in ((ka, 'K_a'), (ba, 'b_a'), (kb, 'K_b')):
        assert np.array_equal(C.bits(got).ravel(), C.bits(want[key]).ravel()), key
    b0, b1 = LARGE_SEP_BIAS_SUM[1]
    with np.errstate(all='ignore'):
        assert np.array_equal(C.bits(bb), C.bits(t[b0] + t[b1]))
    back = split_large_sep_grads(ka, ba, kb, bb, 2)
    assert list(back) != [] and set(back) == set(t)
    for n in t:
        assert back[n].shape == t[n].shape
        assert np.array_equal(C.bits(back[n]), C.bits(bb if n in (b0, b1) else t[n])), n


def test_unknown_group_is_refused():
    from xdet import InvalidArgumentError
    from xdet.train import merged_layout
    with pytest.raises(InvalidArgumentError, match='merged_layout: group must be'):
        merged_layout('stem')
