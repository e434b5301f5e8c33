"""xdet_crc32c on the GPU (xdet.ops.crc32c_device): the CRC-32C of a table of device buffers and their copy in the same pass,
against the NumPy statement xdet.tf_checkpoint.crc32c.  A few MB in all; C is the chunk length the kernel cuts slots into, and
the lengths straddle every boundary the kernel has: the dword, the 128-byte unit a lane owns, the chunk, a slot over many
workgroups (40 C + 1: a fold tree of 64 lanes) and a slot of more than 256 full chunks (the fold's Horner step, G = 2)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KNOWN = [(b'123456789', 0xe3069283), (bytes(32), 0x8a9136aa), (b'\xff' * 32, 0x62a8ab43), (bytes(range(32)), 0x46dd794e), (b'', 0)]


def upload(raw):
    """bytes -> (DeviceBuffer, bytes): the buffer holds them from its first byte"""
    from xdet.runtime import to_device
    n = len(raw)
    a = np.zeros(max((n + 3) // 4 * 4, 16), np.uint8)
    a[:n] = np.frombuffer(raw, np.uint8)
    return to_device(a), n


def device_crcs(raws, **kw):
    from xdet.ops import crc32c_device
    bufs = [upload(r) for r in raws]
    return crc32c_device([(b, n) for b, n in bufs], **kw)


def host_crcs(raws):
    from xdet.tf_checkpoint import crc32c
    return np.array([crc32c(r) if len(r) else 0 for r in raws], np.uint32)


@pytest.fixture(scope='module')
def C():
    from xdet._lib import lib
    c = int(lib().xdet_crc32c_chunk_bytes())
    assert c > 0 and c % 16 == 0
    return c


def lengths(C):
    return [0, 1, 2, 3, 4, 5, 7, 63, 64, 65, 127, 128, 129, C - 1, C, C + 1, 2 * C + 3, 40 * C + 1]


def test_known_answers():
    from xdet.tf_checkpoint import crc32c
    for raw, want in KNOWN:
        assert (crc32c(raw) if raw else 0) == want            # (the statement itself)
    got = device_crcs([raw for raw, _ in KNOWN])
    assert got.dtype == np.uint32 and [int(x) for x in got] == [w for _, w in KNOWN], [hex(int(x)) for x in got]


@pytest.mark.parametrize('content', ['random', 'zero', 'ff'])
def test_every_length_in_one_table(C, content):
    rng = np.random.RandomState(5)
    fill = {'random': lambda n: rng.randint(0, 256, n).astype(np.uint8), 'zero': lambda n: np.zeros(n, np.uint8),
            'ff': lambda n: np.full(n, 255, np.uint8)}[content]
    raws = [fill(n).tobytes() for n in lengths(C)]
    got, want = device_crcs(raws), host_crcs(raws)
    assert got.tolist() == want.tolist(), [(len(r), hex(int(g)), hex(int(w))) for r, g, w in zip(raws, got, want) if g != w]
    if content == 'zero':                                     # leading zeros count: every length has its own CRC
        assert len(set(want.tolist())) == len(raws)


def test_a_slot_of_more_than_256_full_chunks(C):
    raw = np.random.RandomState(6).randint(0, 256, 300 * C + 130).astype(np.uint8).tobytes()
    assert device_crcs([raw]).tolist() == host_crcs([raw]).tolist()


def test_300_small_slots_in_one_table():
    rng = np.random.RandomState(7)
    raws = [rng.randint(0, 256, 4 * rng.randint(1, 10)).astype(np.uint8).tobytes() for _ in range(300)]
    assert {len(r) for r in raws} == set(range(4, 40, 4))
    assert device_crcs(raws).tolist() == host_crcs(raws).tolist()


def test_a_source_that_is_4_but_not_16_byte_aligned(C):
    from xdet.ops import crc32c_device
    raw = np.random.RandomState(8).randint(0, 256, 2 * C + 64).astype(np.uint8).tobytes()
    buf, n = upload(raw)
    assert buf.ptr % 16 == 0
    spans = [(off, ln) for off in (4, 8, 12) for ln in (0, 1, 129, C + 7, 2 * C + 9)]
    got = crc32c_device([(buf.ptr + off, ln) for off, ln in spans])
    assert got.tolist() == host_crcs([raw[off:off + ln] for off, ln in spans]).tolist()
    del buf


def test_copy_is_bit_exact_and_writes_nothing_outside(C):
    """copy mode: NaN payloads, -0 and denormals arrive as they left; guard bytes around every destination stay; slots with and
    without a destination share the table; 16-byte and 4-byte aligned destinations"""
    from xdet.ops import crc32c_device
    from xdet.runtime import to_device, to_host
    rng = np.random.RandomState(9)
    GUARD = 32
    cases = []                                                # (bytes, destination offset inside its guarded buffer or None)
    special = np.array([0x7fc00001, 0xffc12345, 0x7f800001, 0x80000000, 0x00000001, 0x807fffff, 0x7f800000, 0xff800000], np.uint32)
    for n, off in [(0, 0), (1, 0), (3, 4), (5, 0), (127, 12), (128, 0), (129, 4), (C - 1, 0), (C + 1, 8), (2 * C + 3, 0), (3 * C + 70, 4),
                   (260, None), (C + 5, None)]:
        raw = rng.randint(0, 256, n).astype(np.uint8)
        k = min(n // 4, special.size)
        raw[:4 * k] = special[:k].view(np.uint8)
        cases.append((raw.tobytes(), off))
    srcs = [upload(r) for r, _ in cases]
    dsts = []
    for raw, off in cases:
        if off is None:
            dsts.append(None)
            continue
        room = GUARD + off + (len(raw) + 3) // 4 * 4 + GUARD
        dsts.append(to_device(np.full(room, 0xa5, np.uint8)))
    got = crc32c_device([(b, n) for b, n in srcs], copy_to=[None if d is None else d.ptr + GUARD + off for d, (_, off) in zip(dsts, cases)])
    assert got.tolist() == host_crcs([r for r, _ in cases]).tolist()
    for (raw, off), d in zip(cases, dsts):
        if d is None:
            continue
        back = to_host(d.ptr, (d.nbytes,), np.uint8)
        lo = GUARD + off
        assert back[lo:lo + len(raw)].tobytes() == raw, len(raw)
        assert (back[:lo] == 0xa5).all() and (back[lo + len(raw):] == 0xa5).all(), len(raw)


def test_a_second_call_reuses_the_workspace(C):
    from xdet.ops import crc32c_table, crc32c_launch
    from xdet.runtime import DeviceBuffer, to_host, synchronize
    rng = np.random.RandomState(10)
    raws = [rng.randint(0, 256, n).astype(np.uint8).tobytes() for n in (5 * C + 9, 17, 0, C)]
    bufs = [upload(r) for r in raws]
    table, keep = crc32c_table([(b, n) for b, n in bufs])
    out1, out2 = DeviceBuffer(16), DeviceBuffer(16)
    ws = crc32c_launch(table, out1, keep=keep)
    other, _ = crc32c_table([(bufs[3][0], C), (bufs[1][0], 16)])       # another table through the same workspace in between
    crc32c_launch(other, DeviceBuffer(16), workspace=ws)
    crc32c_launch(table, out2, workspace=ws, keep=keep)
    synchronize()
    want = host_crcs(raws).tolist()
    assert to_host(out1.ptr, (4,), np.uint32).tolist() == want and to_host(out2.ptr, (4,), np.uint32).tolist() == want
