"""Write tests/golden/jpeg_cases.npz: for every case the JPEG bytes Pillow (libjpeg-turbo) encodes from seeded random
uint8 content, and the pixels Pillow decodes from those bytes -- the yardstick of xdet/jpeg.py and the decode kernels.
Runs once, where Pillow is installed; no test needs Pillow.  A fixture is data: encoded bytes and pixels only.

    python tests/golden/make_jpeg_fixtures.py
"""
import io
import os

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))

# name: (H, W, mode, save arguments); subsampling 0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0
CASES = [
    ('s444_9x7_q90', 9, 7, 'RGB', dict(subsampling=0, quality=90)),
    ('s422_17x33_q75', 17, 33, 'RGB', dict(subsampling=1, quality=75)),
    ('s422_5x1', 5, 1, 'RGB', dict(subsampling=1)),
    ('s420_37x50_q50', 37, 50, 'RGB', dict(subsampling=2, quality=50)),
    ('s420_15x31_q95', 15, 31, 'RGB', dict(subsampling=2, quality=95)),
    ('s420_40x48_rst2', 40, 48, 'RGB', dict(subsampling=2, restart_marker_blocks=2)),
    ('gray_19x21', 19, 21, 'L', dict()),
    ('s420_1x1', 1, 1, 'RGB', dict(subsampling=2)),
    ('s420_16x16_q100', 16, 16, 'RGB', dict(subsampling=2, quality=100)),
    ('s420_24x24_q3', 24, 24, 'RGB', dict(subsampling=2, quality=3)),
    ('s420_33x17_opt', 33, 17, 'RGB', dict(subsampling=2, optimize=True)),
    ('s420_16x16_progressive', 16, 16, 'RGB', dict(subsampling=2, progressive=True)),      # bytes only: the refusal
    # one or two chroma columns: libjpeg replicates there instead of filtering (jdsample.c: downsampled_width > 2)
    ('s420_9x1', 9, 1, 'RGB', dict(subsampling=2, quality=90)),
    ('s420_9x4', 9, 4, 'RGB', dict(subsampling=2, quality=90)),
    ('s422_5x3', 5, 3, 'RGB', dict(subsampling=1, quality=90)),
    ('s420_17x2', 17, 2, 'RGB', dict(subsampling=2, quality=90)),
    ('s420_6x5', 6, 5, 'RGB', dict(subsampling=2, quality=90)),      # three chroma columns: the narrowest filtered image
]


def content(rng, H, W, mode):
    """smooth content plus noise: low and high frequencies both carry coefficients"""
    c = 1 if mode == 'L' else 3
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.stack([127 + 100 * np.sin(0.3 * xx + k) * np.cos(0.2 * yy - k) for k in range(c)], -1)
    a = np.clip(base + rng.integers(-60, 61, (H, W, c)), 0, 255).astype(np.uint8)
    return a[:, :, 0] if mode == 'L' else a


if __name__ == '__main__':
    rng = np.random.default_rng(20240607)
    out = {'names': np.array([c[0] for c in CASES])}
    for name, H, W, mode, args in CASES:
        buf = io.BytesIO()
        Image.fromarray(content(rng, H, W, mode), mode).save(buf, 'JPEG', **args)
        data = buf.getvalue()
        out[name + '/jpeg'] = np.frombuffer(data, np.uint8)
        if 'progressive' not in name:
            pix = np.asarray(Image.open(io.BytesIO(data)).convert('RGB'), np.uint8)
            assert pix.shape == (H, W, 3), (name, pix.shape)
            out[name + '/pixels'] = pix
        print('%-24s %5d bytes' % (name, len(data)))
    path = os.path.join(HERE, 'jpeg_cases.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')
