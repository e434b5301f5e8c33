#!/usr/bin/env python
"""Golden vectors for RotatedPsRoiAlign / RotatedPsRoiAlignGrad from the REFERENCE's own CPU functors.

    python tests/golden/make_rotated_psroi_golden.py <checkout of HiKapok/X-Detector>

Run by hand on a machine that has the reference; no test runs it.  The reference's two op files
(cpp/PSROIPooling/rotated_ps_roi_align_op.cc, rotated_ps_roi_align_grad_op.cc) are compiled with g++ in a temporary
directory against a small stand-in for the TensorFlow headers written there (just enough declarations for the files
to compile; the op registrations become no-ops and Shard() runs the work in one sequential call), and their CPU
functors are driven through two extern "C" entry points.  Nothing compiled and no reference text is kept: only the
inputs and the functors' outputs go to tests/golden/rotated_psroi_golden.npz.

Every quad of a case keeps all its samples inside the map (checked with tests/rotated_psroi_ref.py): outside it the
reference reads outside the plane, and the product's clamping rule is tested on the GPU instead."""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import rotated_psroi_ref as RR                               # noqa: E402

STUB = r'''
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <functional>
#include <initializer_list>
#include <limits>
#include <string>
#include <tuple>
#include <vector>
namespace Eigen { struct ThreadPoolDevice {}; struct GpuDevice {}; }
namespace tensorflow {
typedef int64_t int64;
typedef int32_t int32;
namespace thread { struct ThreadPool {}; }
struct Status { static Status OK() { return Status(); } bool ok() const { return true; } };
namespace errors { template <typename... A> Status InvalidArgument(const A&...) { return Status(); } }
struct StringPiece {
  std::string s;
  StringPiece(const std::string& x) : s(x) {}
  StringPiece(const char* x) : s(x) {}
  bool contains(const StringPiece& o) const { return s.find(o.s) != std::string::npos; }
};
template <typename T> struct TTypes {
  struct Flat {
    T* p; int64_t n;
    T* data() const { return p; }
    int64_t size() const { return n; }
    Flat& setZero() { std::fill(p, p + n, T(0)); return *this; }
  };
  struct ConstFlat {
    const T* p; int64_t n;
    const T* data() const { return p; }
    int64_t size() const { return n; }
  };
};
struct TensorShape {
  std::vector<int64_t> d;
  TensorShape() {}
  TensorShape(std::initializer_list<int64_t> l) : d(l) {}
  int dims() const { return (int)d.size(); }
  int64_t dim_size(int i) const { return d[i]; }
  bool operator==(const TensorShape& o) const { return d == o.d; }
};
struct Tensor {
  TensorShape sh;
  const TensorShape& shape() const { return sh; }
  int64_t dim_size(int i) const { return sh.dim_size(i); }
  template <typename T> typename TTypes<T>::Flat flat() { return {nullptr, 0}; }
  template <typename T> typename TTypes<T>::ConstFlat flat() const { return {nullptr, 0}; }
};
struct DeviceBase {
  struct CpuWorkerThreads { int num_threads = 1; thread::ThreadPool* workers = nullptr; };
  CpuWorkerThreads w;
  const CpuWorkerThreads* tensorflow_cpu_worker_threads() const { return &w; }
};
struct OpKernelConstruction {
  Status GetAttr(const char*, int32_t*) { return Status(); }
  Status GetAttr(const char*, std::string*) { return Status(); }
};
struct OpKernelContext {
  DeviceBase dev; Tensor t;
  DeviceBase* device() { return &dev; }
  const Tensor& input(int) { return t; }
  Status allocate_output(int, const TensorShape&, Tensor**) { return Status(); }
  template <typename D> const D& eigen_device() { static D d; return d; }
};
struct OpKernel { explicit OpKernel(OpKernelConstruction*) {} virtual ~OpKernel() {} virtual void Compute(OpKernelContext*) = 0; };
namespace shape_inference {
struct ShapeHandle {};
struct DimensionHandle {};
struct DimensionOrConstant { DimensionOrConstant(DimensionHandle) {} DimensionOrConstant(int64_t) {} };
struct InferenceContext {
  ShapeHandle input(int) { return {}; }
  DimensionHandle Dim(ShapeHandle, int) { return {}; }
  Status GetAttr(const char*, int32_t*) { return Status(); }
  Status Divide(DimensionHandle, int64_t, bool, DimensionHandle*) { return Status(); }
  ShapeHandle MakeShape(std::initializer_list<DimensionOrConstant>) { return {}; }
  void set_output(int, ShapeHandle) {}
};
}
struct OpBuilder {
  OpBuilder& Attr(const char*) { return *this; }
  OpBuilder& Input(const char*) { return *this; }
  OpBuilder& Output(const char*) { return *this; }
  OpBuilder& Doc(const char*) { return *this; }
  template <typename F> OpBuilder& SetShapeFn(F) { return *this; }
};
void Shard(int, thread::ThreadPool*, int64 total, int64, std::function<void(int64, int64)> work);
}
#define XDET_CAT2(a, b) a##b
#define XDET_CAT(a, b) XDET_CAT2(a, b)
#define REGISTER_OP(name) static ::tensorflow::OpBuilder XDET_CAT(op_builder_, __COUNTER__) = ::tensorflow::OpBuilder()
#define REGISTER_KERNEL_BUILDER(...)
#define TF_RETURN_IF_ERROR(e) do { ::tensorflow::Status _s = (e); if (!_s.ok()) return _s; } while (0)
#define OP_REQUIRES_OK(ctx, e) do { (void)(e); } while (0)
#define OP_REQUIRES(ctx, cond, err) do { if (!(cond)) { (void)(err); return; } } while (0)
'''

HEADERS = ['third_party/eigen3/unsupported/Eigen/CXX11/Tensor', 'tensorflow/core/framework/tensor_types.h',
           'tensorflow/core/framework/op_kernel.h', 'tensorflow/core/framework/register_types.h',
           'tensorflow/core/framework/tensor.h', 'tensorflow/core/framework/tensor_shape.h',
           'tensorflow/core/framework/op.h', 'tensorflow/core/framework/shape_inference.h',
           'tensorflow/core/lib/core/threadpool.h', 'tensorflow/core/platform/types.h']

DRIVER_FWD = r'''
#include "rotated_ps_roi_align_op.cc"
namespace tensorflow {
void Shard(int, thread::ThreadPool*, int64 total, int64, std::function<void(int64, int64)> work) { work(0, total); }
}
extern "C" void ref_rotated_fwd(const float* in, const float* rois, const int32_t* orders, int N, int C, int H, int W,
                                int R, int gw, int gh, int use_max, float* out, int32_t* idx) {
  OpKernelContext ctx;
  const int64_t n_out = (int64_t)N * R * C;
  RotatedPSROIAlignFunctor<CPUDevice, float>()(&ctx, ctx.eigen_device<CPUDevice>(), {in, (int64_t)N * C * H * W},
      {rois, (int64_t)N * R * 8}, {orders, (int64_t)N * R}, gw, gh, {out, n_out}, {idx, n_out},
      std::make_tuple(N, C, H, W, R, use_max != 0));
}
'''

DRIVER_GRAD = r'''
#include "rotated_ps_roi_align_grad_op.cc"
extern "C" void ref_rotated_grad(const float* in, const float* rois, const int32_t* orders, const float* grad,
                                 const int32_t* idx, int N, int C, int H, int W, int R, int gw, int gh, int use_max,
                                 float* out) {
  OpKernelContext ctx;
  const int64_t n_out = (int64_t)N * R * C, n_in = (int64_t)N * C * H * W;
  RotatedPSROIAlignGradFunctor<CPUDevice, float>()(&ctx, ctx.eigen_device<CPUDevice>(), {in, n_in},
      {rois, (int64_t)N * R * 8}, {orders, (int64_t)N * R}, gw, gh, {grad, n_out}, {idx, n_out}, {out, n_in},
      std::make_tuple(N, C, H, W, R, use_max != 0));
}
'''


def build_reference(ref_root, tmp):
    src = os.path.join(ref_root, 'cpp', 'PSROIPooling')
    for h in HEADERS:
        p = os.path.join(tmp, h)
        os.makedirs(os.path.dirname(p), exist_ok=True)
        open(p, 'w').write('#include "tf_stub.h"\n')
    open(os.path.join(tmp, 'tf_stub.h'), 'w').write(STUB)
    objs = []
    for name, text in (('drv_fwd.cc', DRIVER_FWD), ('drv_grad.cc', DRIVER_GRAD)):
        p = os.path.join(tmp, name)
        open(p, 'w').write(text)
        o = p[:-3] + '.o'
        # baseline x86-64 (no FMA): every a*b+c is two roundings, as in the reference's build
        subprocess.check_call(['g++', '-O2', '-std=c++14', '-fPIC', '-ffp-contract=off', '-w', '-I', tmp, '-I', src,
                               '-c', p, '-o', o])
        objs.append(o)
    so = os.path.join(tmp, 'libref_rotated.so')
    subprocess.check_call(['g++', '-shared', '-o', so] + objs)
    lib = ctypes.CDLL(so)
    P = ctypes.c_void_p
    lib.ref_rotated_fwd.argtypes = [P, P, P] + [ctypes.c_int] * 8 + [P, P]
    lib.ref_rotated_grad.argtypes = [P, P, P, P, P] + [ctypes.c_int] * 8 + [P]
    return lib


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def run(lib, inp, rois, orders, gw, gh, use_max, grad):
    N, C, H, W = inp.shape
    R = rois.shape[1]
    G = gw * gh
    out = np.zeros((N, R, G, C // G), np.float32)
    idx = np.zeros((N, R, G, C // G), np.int32)
    lib.ref_rotated_fwd(ptr(inp), ptr(rois), ptr(orders), N, C, H, W, R, gw, gh, use_max, ptr(out), ptr(idx))
    g_in = np.zeros_like(inp)
    lib.ref_rotated_grad(ptr(inp), ptr(rois), ptr(orders), ptr(grad), ptr(idx), N, C, H, W, R, gw, gh, use_max,
                         ptr(g_in))
    return out, idx, g_in


def rect(cy, cx, h, w, ang):
    """rotated rectangle (normalised), vertices clockwise in (y, x) with y down"""
    c, s = np.cos(ang), np.sin(ang)
    pts = []
    for dy, dx in ((-h / 2, -w / 2), (-h / 2, w / 2), (h / 2, w / 2), (h / 2, -w / 2)):
        pts += [cy + dy * c + dx * s, cx - dy * s + dx * c]
    return pts


def quads(rng, n, H, W):
    """a mix of every kind of quad the fixture covers, all samples in bounds"""
    out = []
    px = 1. / max(H, W)
    while len(out) < n:
        k = len(out) % 8
        if k == 0:             # rotated rectangles at many angles
            q = rect(rng.uniform(0.3, 0.7), rng.uniform(0.3, 0.7), rng.uniform(0.05, 0.6), rng.uniform(0.05, 0.6),
                     rng.uniform(-np.pi, np.pi))
        elif k == 1:           # large ones (several samples per bin), cut by the map's edges into general quads
            q = rect(rng.uniform(0.4, 0.6), rng.uniform(0.4, 0.6), rng.uniform(0.8, 1.3), rng.uniform(0.8, 1.3),
                     rng.uniform(-np.pi, np.pi))
        elif k == 2:           # general convex: jittered rectangle
            q = list(np.array(rect(rng.uniform(0.3, 0.7), rng.uniform(0.3, 0.7), 0.4, 0.3, rng.uniform(0, np.pi)))
                     + rng.uniform(-0.06, 0.06, 8))
        elif k == 3:           # concave: one vertex pulled past the centre
            q = rect(0.5, 0.5, rng.uniform(0.2, 0.6), rng.uniform(0.2, 0.6), rng.uniform(0, np.pi))
            q[4], q[5] = 0.5 + 0.6 * (0.5 - q[4]) * rng.uniform(0.1, 0.9), 0.5 + 0.6 * (0.5 - q[5]) * rng.uniform(0.1, 0.9)
        elif k == 4:           # self-intersecting: two vertices swapped
            q = rect(rng.uniform(0.35, 0.65), rng.uniform(0.35, 0.65), rng.uniform(0.1, 0.5), rng.uniform(0.1, 0.5),
                     rng.uniform(0, np.pi))
            q[2:4], q[4:6] = q[4:6], q[2:4]
        elif k == 5:           # 1-pixel quads
            q = rect(rng.uniform(0.1, 0.9), rng.uniform(0.1, 0.9), px, px, rng.uniform(0, np.pi))
        elif k == 6:           # touching the border (x = 0 / y = 0 exactly, far side just inside)
            q = [0., rng.uniform(0.1, 0.6), rng.uniform(0.2, 0.5), 0.999, 0.999, rng.uniform(0.4, 0.9),
                 rng.uniform(0.3, 0.8), 0.]
        else:                  # axis-aligned box
            y0, x0 = rng.uniform(0.0, 0.5, 2)
            y1, x1 = y0 + rng.uniform(0.05, 0.49), x0 + rng.uniform(0.05, 0.49)
            q = [y0, x0, y0, x1, y1, x1, y1, x0]
        q = np.clip(np.array(q, np.float64), 0., 0.999).astype(np.float32)
        if not RR.out_of_bounds(q.reshape(1, 1, 8), np.array([[-1]]), H, W, 1, 1)[0, 0]:
            out.append(q)
    return np.array(out, np.float32)


def degenerate(rng, n):
    """repeated vertex: one side of length 0"""
    q = quads(rng, n, 9, 11).reshape(n, 4, 2)
    k = rng.integers(0, 4, n)
    q[np.arange(n), (k + 1) % 4] = q[np.arange(n), k]
    return q.reshape(n, 8)


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref_root = sys.argv[1]
    rng = np.random.default_rng(20181016)
    store = {}
    with tempfile.TemporaryDirectory() as tmp:
        lib = build_reference(ref_root, tmp)
        # 1. the reference's own test inputs (cpp/PSROIPooling/test_op.py:133-141)
        plane = np.arange(1, 26, dtype=np.float32).reshape(5, 5)
        kat_in = np.ascontiguousarray(np.tile(plane, (1, 16, 1, 1)), np.float32)
        kat_rois = np.array([[[0.1, 0.1, 0.2, 0.3, 0.5, 0.5, 0.3, 0.2], [0.5, 0.5, 0.6, 0.7, 0.9, 0.9, 0.7, 0.6],
                              [0.6, 0.7, 0.9, 0.9, 0.7, 0.6, 0.2, 0.2]]], np.float32)
        kat_orders = np.array([[1, -1, 0]], np.int32)
        cases = [('kat', kat_in, kat_rois, kat_orders, 2, 2, np.ones((1, 3, 4, 4), np.float32))]
        # 2. seeded maps: 7 x 7 grid over 49 channels, and a non-square 3 x 2 grid (catches width / height swaps)
        for name, (N, C, H, W, gw, gh, R) in (('g7', (2, 49, 9, 11, 7, 7, 24)), ('g32', (2, 12, 9, 11, 3, 2, 40))):
            inp = rng.standard_normal((N, C, H, W)).astype(np.float32)
            rois = quads(rng, N * R, H, W).reshape(N, R, 8)
            rois[:, -3:] = degenerate(rng, N * 3).reshape(N, 3, 8)
            orders = rng.integers(-1, 4, (N, R)).astype(np.int32)
            orders[:, :5] = np.arange(-1, 4)                       # every order in {-1, 0, 1, 2, 3}
            G = gw * gh
            grad = rng.uniform(-1, 1, (N, R, G, C // G)).astype(np.float32)
            cases.append((name, inp, rois, orders, gw, gh, grad))
        for name, inp, rois, orders, gw, gh, grad in cases:
            assert not RR.out_of_bounds(rois, orders, inp.shape[2], inp.shape[3], gw, gh).any(), name
            store[name + '_inputs'] = inp
            store[name + '_rois'] = rois
            store[name + '_orders'] = orders
            store[name + '_grid'] = np.array([gw, gh], np.int32)
            store[name + '_grad'] = grad
            for method, use_max in (('mean', 0), ('max', 1)):
                out, idx, g_in = run(lib, inp, rois, orders, gw, gh, use_max, grad)
                store['%s_%s_pooled' % (name, method)] = out
                store['%s_%s_index' % (name, method)] = idx
                store['%s_%s_grad_inputs' % (name, method)] = g_in
                print('%-4s %-4s pooled %s  index max %d  grad sum %.6f' % (name, method, out.shape, idx.max(),
                                                                             float(g_in.astype(np.float64).sum())))
    path = os.path.join(HERE, 'rotated_psroi_golden.npz')
    np.savez_compressed(path, **store)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
