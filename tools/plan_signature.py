#!/usr/bin/env python
"""What a net's builders decided, as one JSON object per configuration: every op of the launch plan (name, FLOPs per image,
issued MFMA FLOPs), the activation pre-scale entries in order, and the workspace's allocated / recycled bytes.  Two builds of
the library that print the same bytes plan the same ops in the same order over the same workspace blocks -- the check for a
change to the builders that must not change what they decide.  XDET_LIB selects another build, as with tools/ab.sh -l.
Needs a GPU (building a net allocates its workspace).

  tools/plan_signature.py --net lighthead --size 480 --batch 8 --proposals 300 --opt ksplit=all
  tools/plan_signature.py --net resnet50 --sweep       (default, f32, and every option value other than its default)
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'x-detector_amd'))

from xdet import weights as W                                   # noqa: E402
from xdet._lib import lib, check, c_void_p, LightHeadConfig     # noqa: E402
from xdet.runtime import set_precision, _host                   # noqa: E402
import numpy as np                                              # noqa: E402

# every value of every xdet_net_set_option / xdet_resnet_set_option key other than its default
SWEEP = {
    'lighthead': [('large_sep', 'direct'), ('large_sep', 'spectral'), ('rpn_stream', 'main'), ('pool_sub', 'off'),
                  ('workspace', 'ssa'), ('workspace', 'poison'), ('sepconv', 'split'), ('ksplit', 'off'), ('ksplit', 'all'),
                  ('cross', 'fp8'), ('check_range', 'on'), ('pool', 'whole'), ('pool', 'split_all'), ('conv3x3', 'gemm')],
    'resnet50': [(k, 'off') for k in ('ksplit', 'stem7', 'stem_pool', 'bneck', 'projcat', 'preconv')],
}


def signature(net, precision, size, batch, proposals, options, weights):
    L = lib()
    set_precision(precision)
    h = c_void_p()
    if net == 'lighthead':
        kind, pre = 0, 'xdet_net_'
        cfg = LightHeadConfig(image_size=size, max_batch=batch, rpn_post_nms_top_n=proposals)
        check(L.xdet_net_create(ctypes.byref(h), ctypes.byref(cfg)))
    else:
        kind, pre = 1, 'xdet_resnet_'
        check(L.xdet_resnet_create(ctypes.byref(h), size, batch))
    try:
        for k, v in options:
            check(getattr(L, pre + 'set_option')(h, k.encode(), v.encode()))
        for name, arr in weights.items():
            a = np.ascontiguousarray(arr, np.float32)
            check(getattr(L, pre + 'set_weight')(h, name.encode(), _host(a), a.ndim, (ctypes.c_int64 * a.ndim)(*a.shape)))
        check(getattr(L, pre + 'build')(h))
        n = ctypes.c_int()
        cap = 4096
        ms, launches = (ctypes.c_double * cap)(), (ctypes.c_int * cap)()
        flops, issued = (ctypes.c_double * cap)(), (ctypes.c_double * cap)()
        check(L.xdet_profile_read(h, kind, cap, ctypes.byref(n), ms, launches, flops))   # (profiling off: names and flops only)
        check(L.xdet_profile_mfma_flops(h, kind, cap, ctypes.byref(n), issued))
        buf = ctypes.create_string_buffer(512)
        ops = []
        for i in range(n.value):
            check(L.xdet_profile_op_name(h, kind, i, buf, 512))
            ops.append({'name': buf.value.decode(), 'flops': flops[i], 'mfma_flops': issued[i]})
        check(L.xdet_net_plane_scales(h, 0, ctypes.byref(n), None))
        pscales = []
        for i in range(n.value):
            check(L.xdet_net_plane_scale_name(h, i, buf, 512))
            pscales.append(buf.value.decode())
        a, r = ctypes.c_size_t(), ctypes.c_size_t()
        check(L.xdet_net_memory(h, ctypes.byref(a), ctypes.byref(r)))
    finally:
        getattr(L, pre + 'destroy')(h)
    return {'net': net, 'precision': precision, 'image_size': size, 'max_batch': batch,
            'proposals': proposals if net == 'lighthead' else None, 'options': dict(options), 'ops': ops, 'pscales': pscales,
            'allocated_bytes': int(a.value), 'recycled_bytes': int(r.value)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--net', choices=('lighthead', 'resnet50'), default='lighthead')
    ap.add_argument('--precision', choices=('f32', 'f16x3', 'f16'), default='f16x3')
    ap.add_argument('--size', type=int, default=480)
    ap.add_argument('--batch', type=int, default=8, help='max_batch')
    ap.add_argument('--proposals', type=int, default=300)
    ap.add_argument('--opt', action='append', default=[], metavar='KEY=VALUE')
    ap.add_argument('--sweep', action='store_true', help='one line each: the default, f32, every non-default option value')
    a = ap.parse_args()
    weights = W.make_lighthead_weights(1234) if a.net == 'lighthead' else W.make_resnet50_weights(4321)
    opts = [tuple(o.split('=', 1)) for o in a.opt]
    configs = [(a.precision, opts)]
    if a.sweep:
        configs = [('f16x3', []), ('f32', [])] + [('f16x3', [kv]) for kv in SWEEP[a.net]]
    for precision, options in configs:
        print(json.dumps(signature(a.net, precision, a.size, a.batch, a.proposals, options, weights), sort_keys=True))
        sys.stdout.flush()


if __name__ == '__main__':
    main()
