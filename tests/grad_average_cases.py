"""Shared inputs of the gradient-average tests (tests/test_grad_average_math.py on the CPU, tests/test_gpu_grad_average.py on
the GPU and in its rank processes): a table of slot sizes and every rank's gradients for it, pure NumPy.

With chunk_elems = 1024 the sizes give slots shorter than a vector (1, 3), slots that end on and off a 4-element boundary
(4, 1024 / 5, 1023, 1025, 4095, 4097, 2500 -- so padding of 3, 1, 2 and 0 elements occurs), slots that begin in the middle of
a chunk (every one but the first), a slot that spans more than three chunks (4097 from flat element 7192: chunks 7 to 11), and
a short last chunk (T = 13792 = 13 * 1024 + 480).

Values are standard normal f32 with planted elements (PLANTED: name -> (slot, position)); what a rank holds there:
  zeros       four positions of +-0 combinations, the sign of the sum follows IEEE addition:
              all +0 -> +0;  all -0 -> -0;  -0 on rank 0, +0 elsewhere -> +0 (world > 1);  +0 on rank 0, -0 elsewhere -> +0
  denormals   the smallest denormal on every rank;  (rank + 1) * 1e-40;  the largest denormal on every rank
  inf         +inf on rank 1 alone, on a slot's last element, which lies alone in its vector
  nan         NaN on rank 0 alone, on the last element of a slot that ends one short of a vector
  order       1e8, -1e8, 1 on ranks 0, 1, 2 and +0 above: rank order gives (1e8 + -1e8) + 1 = 1, so the mean is 1 / world for
              world >= 3, while every order that does not start with g0 + g1 loses the 1 against 1e8 and gives 0.  At world 2
              the probe is vacuous (1e8 + -1e8 = 0 in either order) and at world 1 it is 1e8.
"""
import numpy as np

SIZES = [1, 3, 4, 5, 1023, 1024, 1025, 4095, 4097, 2500]
CHUNK = 1024
SEED = 20240611

PLANTED = {'zeros': (4, 0), 'denormals': (5, 0), 'inf': (6, 1024), 'nan': (7, 4094), 'order': (8, 4096)}

_ORDER = (1e8, -1e8, 1.0)


def rank_grads(rank, sizes=SIZES, seed=SEED):
    """-> rank `rank`'s gradients for `sizes`, a list of f32 vectors; the planted elements go where PLANTED says whenever the
    table is SIZES (a table that differs in one size keeps the rest)"""
    rng = np.random.default_rng([int(seed), int(rank)])
    grads = [rng.standard_normal(int(n)).astype(np.float32) for n in sizes]
    if list(sizes[:9]) != SIZES[:9]:
        return grads
    pz, nz = np.float32(0.0), np.float32(-0.0)
    s, p = PLANTED['zeros']
    grads[s][p:p + 4] = [pz, nz, nz if rank == 0 else pz, pz if rank == 0 else nz]
    s, p = PLANTED['denormals']
    grads[s][p:p + 3] = np.array([1, (rank + 1) * 71362, 0x007fffff], np.uint32).view(np.float32)     # 71362 * 2^-149 ~ 1e-40
    s, p = PLANTED['inf']
    if rank == 1:
        grads[s][p] = np.inf
    s, p = PLANTED['nan']
    if rank == 0:
        grads[s][p] = np.nan
    s, p = PLANTED['order']
    grads[s][p] = _ORDER[rank] if rank < 3 else 0.0
    return grads


def same_bits(a, b):
    """a and b, f32 arrays of one shape, hold the same bits -- NaN positions are compared by isnan alone"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))
