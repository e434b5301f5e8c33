"""The order-exact PsRoiAlign gradient without a GPU: the C door exists in the header, the ctypes table and the library, it
refuses bad arguments before touching a device, and the oracle's gradient really is the sequential order the kernel
promises -- so that `array_equal` against it on the GPU (tests/test_gpu_psroialign_grad_ordered.py) can tell orders apart."""
import os
import re
import subprocess

import numpy as np
import pytest

import psroi_grad_ordered_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('xdet_psroialign_grad_ordered', 'xdet_net_head_pool_backward')


def test_new_symbols_in_header_ctypes_and_library():
    from xdet import _lib, build
    hdr = open(os.path.join(ROOT, 'include', 'xdet.h')).read()
    exported = subprocess.check_output(['nm', '-D', '--defined-only', build.build()]).decode()
    for name in NEW:
        assert re.search(r'\b%s\s*\(' % name, hdr), name
        assert name in _lib.SIGNATURES
        assert re.search(r'\sT\s+%s\b' % name, exported), name
    m = re.search(r'#define XDET_PSROIALIGN_GRAD_ORDERED_MAX_PIXELS (\d+)', hdr)
    assert m and 100 * 100 <= int(m.group(1)) < 512 * 512
    assert b'psroialign_grad_ordered_kernel' in open(build.build(), 'rb').read()


def test_c_door_refuses_before_any_gpu_work():
    """every refusal of include/xdet.h, with pointers that are never dereferenced"""
    from xdet._lib import lib
    l = lib()
    for kw in PC.REFUSALS:
        assert PC.c_call(l, **kw) == -1, kw
        assert b'psroialign_grad_ordered' in l.xdet_last_error(), kw
    # 'mean' may leave the index out -- but the other checks still hold for it
    assert PC.c_call(l, use_max=0, index=None, ld_index=0, ld_grad=15) == -1
    assert PC.c_call(l, use_max=0, index=None, ld_index=0, H=512, W=512) == -1
    # a net handle is checked before anything else
    assert l.xdet_net_head_pool_backward(None, 1, PC.P, 16, PC.P, None) == -1


def test_python_door_refuses_before_any_gpu_work():
    import xdet
    z = np.zeros
    with pytest.raises(xdet.InvalidArgumentError):
        xdet.ps_roi_align_grad(z((1, 18, 4, 4), np.float32), z((1, 2, 4)), z((1, 2, 18)), z((1, 2, 18)), 2, 2, 'max', ordered=True)
    with pytest.raises(xdet.InvalidArgumentError):
        xdet.ps_roi_align_grad(z((1, 16, 4, 4), np.float32), z((1, 2, 4)), z((1, 2, 16)), z((1, 2, 16)), 2, 2, 'median', ordered=True)
    with pytest.raises(xdet.InvalidArgumentError):
        xdet.ps_roi_align_grad_device(z((1, 2, 4)), z((1, 2, 16)), None, (1, 4, 4, 16), 2, 2, 'max')
    with pytest.raises(xdet.InvalidArgumentError):
        xdet.ps_roi_align_grad_device(z((1, 2, 4)), z((1, 2, 18)), z((1, 2, 18)), (1, 4, 4, 18), 2, 2, 'max')


@pytest.mark.parametrize('method', ['max', 'mean'])
def test_oracle_gradient_is_the_sequential_order(method, oracle):
    rois, grad, index, ref = PC.case(PC.SMALL, method, oracle)
    assert ref.any()
    assert np.array_equal(PC.grad_np(rois, grad, index, PC.SMALL, method), ref)


def test_another_roi_order_gives_other_bits(oracle):
    """the heavy-overlap input: the same terms with the ROIs walked backwards round differently, so a kernel that does not
    keep the ROI order cannot pass the GPU test's array_equal"""
    rois, grad, index, ref = PC.case(PC.HEAVY, 'mean', oracle)
    assert np.array_equal(PC.grad_np(rois, grad, index, PC.HEAVY, 'mean'), ref)
    rev = PC.grad_np(rois, grad, index, PC.HEAVY, 'mean', reverse_rois=True)
    assert not np.array_equal(rev, ref)
    assert np.allclose(rev, ref, rtol=1e-4, atol=1e-5)          # ... the same sums to rounding
    print('elements whose bits depend on the ROI order: %d of %d' % ((rev != ref).sum(), ref.size))


def test_corner_conversion_helper_is_the_forwards():
    """hh = y1 - y0; cy = y0 + hh / 2, each step in f32 -- and a degenerate box stays degenerate"""
    rng = np.random.default_rng(PC.SEED)
    corners, centres = PC.corners_of(PC.random_rois(rng, 2, 9))
    assert centres.dtype == np.float32 and np.array_equal(centres[..., 2], corners[..., 2] - corners[..., 0])
    assert (centres[:, 5, 2] == 0).all() and (centres[:, 6, 3] == 0).all()
