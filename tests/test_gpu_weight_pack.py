"""xdet_tensors_concat / xdet_tensors_split (xdet.ops.concat_device / split_device) against their NumPy statements, bit for bit:
the op does no arithmetic, so NaN payloads, -0 and denormals must arrive as they left.  Every slot's source is made of distinct
bit patterns (tests/weight_pack_cases.py) -- an element that lands in another place shows.  Each case runs alone and then all of
them as one table in one launch, every destination followed by a guard band that must keep its fill."""
import numpy as np
import pytest

import weight_pack_cases as C

pytestmark = pytest.mark.gpu
f32 = np.float32
GUARD = 64                                               # floats behind every destination
FILL = np.uint32(0x7FA5A5A5)                              # a NaN no source holds


class Dest(object):
    """a device buffer of `off` + n + GUARD floats filled with FILL; the tensor is the n floats from float `off` on"""

    def __init__(self, n, shape, off=0):
        from xdet.runtime import DeviceTensor, to_device
        self.n, self.off = n, off
        self.buf = to_device(np.full(off + n + GUARD, FILL, np.uint32))
        self.tensor = DeviceTensor(self.buf.ptr + 4 * off, shape, shape[-1], owner=self.buf)

    def read(self):
        """-> (the tensor's bits, everything around it is still the fill)"""
        from xdet.runtime import to_host
        raw = to_host(self.buf.ptr, (self.off + self.n + GUARD,), np.uint32)
        return raw[self.off:self.off + self.n], bool((raw[:self.off] == FILL).all() and (raw[self.off + self.n:] == FILL).all())


def source(a, off=0):
    """a host array on the device, its base `off` floats behind a 16-byte boundary -> a DeviceTensor that owns it"""
    from xdet.runtime import DeviceTensor, to_device
    flat = np.concatenate([np.full(off, FILL, np.uint32), C.bits(a).ravel()])
    buf = to_device(flat)
    return DeviceTensor(buf.ptr + 4 * off, a.shape, a.shape[-1], owner=buf)


def concat_slot(outer, widths, misalign, seed):
    """-> (the slot for concat_device, its destination, the statement's merged bits)"""
    from xdet import host_concat
    parts = C.parts_of(outer, widths, seed)
    dest = Dest(outer * sum(widths), (outer, sum(widths)))
    srcs = [source(p, misalign if i == len(parts) - 1 else 0) for i, p in enumerate(parts)]
    return (dest.tensor, outer, list(zip(srcs, widths))), dest, C.bits(host_concat(parts, outer)).ravel()


def split_slot(outer, widths, misalign, seed):
    """-> (the slot for split_device, its destinations, the statement's parts' bits)"""
    from xdet import host_split
    merged = C.patterns(outer * sum(widths), seed).reshape(outer, sum(widths))
    dests = [Dest(outer * w, (outer, w), misalign if i == len(widths) - 1 else 0) for i, w in enumerate(widths)]
    want = [C.bits(p).ravel() for p in host_split(merged, outer, widths)]
    return (source(merged), outer, [(d.tensor, w) for d, w in zip(dests, widths)]), dests, want


def check(dests, wants, what):
    for i, (d, want) in enumerate(zip(dests, wants)):
        got, guard = d.read()
        assert np.array_equal(got, want), (what, i, int((got != want).sum()), want.size)
        assert guard, (what, i, 'the guard band was written')


@pytest.mark.parametrize('name,outer,widths,misalign', C.CASES, ids=[c[0] for c in C.CASES])
def test_concat_equals_the_statement(name, outer, widths, misalign):
    from xdet import concat_device
    from xdet.runtime import synchronize
    slot, dest, want = concat_slot(outer, widths, misalign, seed=21)
    concat_device([slot])
    synchronize()
    check([dest], [want], name)
    assert 0x80000000 in want and 0x7FC12345 in want and 0xFF812345 in want           # -0 and two NaNs' payloads went through


@pytest.mark.parametrize('name,outer,widths,misalign', C.CASES, ids=[c[0] for c in C.CASES])
def test_split_equals_the_statement(name, outer, widths, misalign):
    from xdet import split_device
    from xdet.runtime import synchronize
    slot, dests, wants = split_slot(outer, widths, misalign, seed=22)
    split_device([slot])
    synchronize()
    check(dests, wants, name)


def test_one_table_in_one_launch_leaves_the_guard_bands():
    """all cases as one table, in both directions, on a stream of their own and with a caller's workspace"""
    from xdet import concat_device, split_device
    from xdet import train_ops
    from xdet._lib import lib
    from xdet.runtime import DeviceBuffer, Stream
    stream = Stream()
    made = [concat_slot(outer, widths, mis, seed=31 + i) for i, (_, outer, widths, mis) in enumerate(C.CASES)]
    table, _ = train_ops._pack_table([m[0] for m in made], 'tensors_concat')
    need = lib().xdet_tensors_concat_workspace_bytes(table, len(table))
    assert need > 0 and need == lib().xdet_tensors_split_workspace_bytes(table, len(table))
    ws = DeviceBuffer(need)
    concat_device([m[0] for m in made], stream=stream, workspace=ws)
    stream.synchronize()
    check([m[1] for m in made], [m[2] for m in made], 'concat table')
    made = [split_slot(outer, widths, mis, seed=51 + i) for i, (_, outer, widths, mis) in enumerate(C.CASES)]
    split_device([m[0] for m in made], stream=stream, workspace=ws)
    stream.synchronize()
    check([d for m in made for d in m[1]], [w for m in made for w in m[2]], 'split table')


def test_two_split_slots_may_read_one_merged_tensor():
    """the adjoint of b0 + b1: both addends get the merged gradient"""
    from xdet import split_device
    from xdet.runtime import synchronize
    g = C.patterns(490, 7)
    src = source(g)
    a, b = Dest(490, (490,)), Dest(490, (490,))
    split_device([(src, 1, [(a.tensor, 490)]), (src, 1, [(b.tensor, 490)])])
    synchronize()
    check([a, b], [C.bits(g), C.bits(g)], 'same source twice')


def test_refusals_come_ahead_of_any_gpu_work():
    """the C doors': an empty table, a NULL pointer, outer <= 0, a width <= 0, more than 4 parts, a NULL workspace -- each
    XDET_ERR_INVALID_ARG with the destination untouched; and the Python doors' own"""
    from xdet import concat_device, split_device, InvalidArgumentError
    from xdet._lib import lib, PackSlot
    from xdet.runtime import DeviceBuffer, synchronize
    l = lib()
    dest, src, ws = Dest(8, (2, 4)), source(C.patterns(8, 1).reshape(2, 4)), DeviceBuffer(4096)

    def slot(merged=None, outer=2, n_parts=1, part=None, width=4):
        s = PackSlot()
        s.merged, s.outer, s.n_parts = dest.tensor.ptr if merged is None else merged, outer, n_parts
        s.part[0], s.width[0] = src.ptr if part is None else part, width
        for i in range(1, 4):
            s.part[i], s.width[i] = src.ptr, 4
        return s
    cases = {'a NULL merged': slot(merged=0), 'a NULL part': slot(part=0), 'outer <= 0': slot(outer=0), 'a width <= 0': slot(width=0),
             'more than 4 parts': slot(n_parts=5), 'no parts': slot(n_parts=0)}
    for door, sizer in ((l.xdet_tensors_concat, l.xdet_tensors_concat_workspace_bytes), (l.xdet_tensors_split, l.xdet_tensors_split_workspace_bytes)):
        for what, s in cases.items():
            table = (PackSlot * 1)(s)
            assert door(table, 1, ws.ptr, None) == -1, what
            assert 'tensors_' in l.xdet_last_error().decode(), what
            assert sizer(table, 1) == 0, what
        good = (PackSlot * 1)(slot())
        assert door(good, 0, ws.ptr, None) == -1 and door(None, 1, ws.ptr, None) == -1          # an empty table
        assert door(good, 1, None, None) == -1 and 'workspace is NULL' in l.xdet_last_error().decode()
        assert sizer(good, 1) > 0
    synchronize()
    got, guard = dest.read()
    assert (got == FILL).all() and guard                                                        # nothing ran
    for door in (concat_device, split_device):
        for bad in ([], [(dest.tensor, 2, [])], [(dest.tensor, 0, [(src, 4)])], [(dest.tensor, 2, [(src, 0)])],
                    [(dest.tensor, 2, [(src, 4)] * 5)], [(dest.tensor, 2, [(np.zeros((2, 4), f32), 4)])],
                    [(dest.tensor, 2, [(src, 3)])], [(dest.tensor, 3, [(src, 4)])]):
            with pytest.raises(InvalidArgumentError):
                door(bad)
        with pytest.raises(InvalidArgumentError):
            door([(dest.tensor, 2, [(src, 4)])], workspace=DeviceBuffer(16))
