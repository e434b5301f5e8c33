"""The host entropy stage (csrc/jpeg_parse.h: marker parser, Huffman decoder) on damaged input, under AddressSanitizer and
UndefinedBehaviorSanitizer: a stand-alone host program (tests/jpeg_parse_check.cpp: its own main, built with the host
compiler from that header alone; nothing is loaded into Python and nothing is preloaded) runs it on every prefix of each
small fixture and on each fixture with every single byte of its first 700 set to 0x00, 0xFF and 0xD9 in turn.  A bad stream
must be a refusal with a message, never an out-of-range access; the valid file is accepted and no prefix that ends inside
the entropy-coded data is."""
import os
import re
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'x-detector_amd', 'csrc')
SMALL = ['s444_9x7_q90', 's422_17x33_q75', 's422_5x1', 's420_37x50_q50', 's420_15x31_q95', 's420_40x48_rst2', 'gray_19x21',
         's420_1x1', 's420_16x16_q100', 's420_24x24_q3', 's420_33x17_opt',
         # one or two chroma columns (replicated, not filtered), and three (the narrowest filtered)
         's420_9x1', 's420_9x4', 's422_5x3', 's420_17x2', 's420_6x5']


def test_entropy_stage_refuses_damaged_streams_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / 'jpeg_parse_check')
    cxx = os.environ.get('CXX', 'c++')
    subprocess.check_call([cxx, '-std=c++17', '-O1', '-g', '-Wall', '-Werror', '-fsanitize=address,undefined',
                           '-fno-sanitize-recover=all', '-I', CSRC, os.path.join(ROOT, 'tests', 'jpeg_parse_check.cpp'), '-o', exe])
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'jpeg_cases.npz'))
    blob = str(tmp_path / 'cases.bin')
    total = prefixes_short = 0
    with open(blob, 'wb') as f:
        for name in SMALL:
            data = z[name + '/jpeg'].tobytes()
            f.write(struct.pack('<I', len(data)) + data)
            total += len(data) + 1 + 3 * min(len(data), 700)
            prefixes_short += len(data) - 2                           # prefixes that miss more than the EOI marker
    r = subprocess.run([exe, blob], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    out, err = r.stdout.decode(), r.stderr.decode()
    assert r.returncode == 0, (out, err)
    assert 'runtime error' not in err and 'AddressSanitizer' not in err, err
    m = re.match(r'ok: (\d+) accepted, (\d+) refused, (\d+) cases', out)
    assert m, out
    accepted, refused, cases = (int(g) for g in m.groups())
    assert cases == len(SMALL) and accepted + refused == total
    # the program itself fails on an accepted short prefix; the counts say that they were all there.  A damaged byte may go
    # either way (most bytes of an APP0 segment or of a quantisation table leave a decodable file), so only the prefixes bound
    # the counts: per case the file and it without one or both bytes of its EOI are accepted, every shorter prefix is refused
    assert accepted >= 3 * len(SMALL) and refused >= prefixes_short
