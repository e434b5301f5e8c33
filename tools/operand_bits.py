#!/usr/bin/env python
"""What the layers compute from their operand buffers, as one line per item: a blake2b of the output's bits.  Two builds of
the library that print the same bytes hold the same operands in every conv layer these items run -- the check for a change
to how the operands are made (csrc/conv_repack.hip) that must not change one bit of them.  XDET_LIB selects another build,
as with tools/ab.sh -l; run each build in a process of its own and compare the outputs with cmp.  Needs a GPU.

Items: every conv case of tests/test_gpu_optimizer.py (its seeds, the layer created from W1) in f32 / f16 / f16x3 through
every forward door; two spectral convs (F 16 and 30, 64 -> 32 channels, their grouped per-bin operands); the light-head
detector at 256 px with large_sep direct and spectral (five of its tensors, the proposals and the detections); the ResNet-50
trunk at 224 px in f16x3 and f32.

  tools/operand_bits.py > new.txt;  XDET_LIB=other/libxdet_hip.so tools/operand_bits.py > other.txt;  cmp new.txt other.txt
"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'x-detector_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np                                                                  # noqa: E402
from xdet import weights as W                                                       # noqa: E402
from xdet.model import LightHeadDetector                                            # noqa: E402
from xdet.ops import Conv2D, SpectralConv                                           # noqa: E402
from xdet.resnet import ResNet50Trunk                                               # noqa: E402
from xdet.runtime import DeviceTensor, set_precision                                # noqa: E402
from test_gpu_optimizer import CONV_CASES, doors, kernels                           # noqa: E402

f32 = np.float32


def emit(name, a):
    a = np.ascontiguousarray(a)
    print('%s %s %s %s' % (name, a.dtype, 'x'.join(map(str, a.shape)), hashlib.blake2b(a.tobytes(), digest_size=16).hexdigest()))
    sys.stdout.flush()


def conv_cases():
    for case in sorted(CONV_CASES):
        kh, kw, cin, cout, affine = CONV_CASES[case]
        for mode in ('f32', 'f16', 'f16x3'):
            w0, w1 = kernels(kh, kw, cin, cout, 5)                                  # (test_conv_refresh_equals_a_fresh_layer's draws)
            rng = np.random.default_rng(9)
            scale = rng.uniform(0.5, 2.0, cout).astype(f32) if affine else None
            sh0, sh1 = ((rng.standard_normal(cout).astype(f32) for _ in range(2)) if affine else (None, None))
            x = DeviceTensor.from_numpy(rng.standard_normal((2, 8, 8, cin)).astype(f32))
            set_precision(mode)
            fresh = Conv2D(w1, scale=scale, shift=sh1)
            for door, b in sorted(doors(fresh, x, mode, kh == kw == 1, cin).items()):
                emit('conv [%s] %s %s' % (case, mode, door), b)


def spectral():
    set_precision('f16x3')
    for F in (16, 30):
        rng = np.random.default_rng(F)
        w = (rng.standard_normal((15, 64, 32)) / np.sqrt(15 * 64)).astype(f32)
        scale, shift = rng.uniform(0.5, 1.5, 32).astype(f32), rng.standard_normal(32).astype(f32)
        x = DeviceTensor.from_numpy(rng.standard_normal((2, F, F, 64)).astype(f32))
        for axis in (0, 1):
            emit('spectral F%d axis %d' % (F, axis), SpectralConv(w, axis, F, scale, shift, relu=True)(x).numpy())


def lighthead():
    set_precision('f16x3')
    weights = W.make_lighthead_weights(1234)
    images = np.random.default_rng(77).standard_normal((2, 3, 256, 256)).astype(f32)
    for large_sep in ('direct', 'spectral'):
        det = LightHeadDetector(weights, image_size=256, max_batch=2, rpn_post_nms_top_n=100, large_sep=large_sep)
        det.forward_device(det.set_images(images))
        scores, boxes = det.detections(2)
        for name in ('mid_x', 'rpn_out', 'out', 'feat', 'cls_reg'):
            emit('lighthead %s %s' % (large_sep, name), det.buffer(name, 2).numpy())
        emit('lighthead %s proposals' % large_sep, det.flat('proposals', (2, 100, 4)))
        emit('lighthead %s det_scores' % large_sep, scores)
        emit('lighthead %s det_boxes' % large_sep, boxes)


def resnet():
    weights = W.make_resnet50_weights(4321)
    images = np.random.default_rng(78).standard_normal((2, 3, 224, 224)).astype(f32)
    for mode in ('f16x3', 'f32'):
        set_precision(mode)
        emit('resnet50 %s' % mode, ResNet50Trunk(weights, image_size=224, max_batch=2).forward(images))


if __name__ == '__main__':
    conv_cases()
    spectral()
    lighthead()
    resnet()
