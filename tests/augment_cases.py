"""The shared case list of the training-ingest tests (test_augment_math.py on the host contract, test_gpu_augment.py on
the kernels): plain data and generators, no test.  A case is (name, image uint8 [H,W,3], labels i32 [g], bboxes f32 [g,4],
seed, image_id)."""
import numpy as np

# the ingest tests' sizes, plus a tiny image (sides below 10: ssd_random_expand's uniform int meets an empty range)
SHAPES = [(333, 500), (500, 375), (480, 480), (97, 1013), (1013, 97), (479, 481), (700, 700), (7, 9)]
SEEDS = [1, 7, 2024, 31337]


def rand_image(H, W, seed=0):
    return np.random.default_rng(seed + 7 * H + W).integers(0, 256, (H, W, 3), dtype=np.uint8)


def _mixed(rng, n):
    """n boxes of mixed sizes inside [0,1], (ymin, xmin, ymax, xmax)"""
    c = rng.uniform(0.15, 0.85, (n, 2))
    s = rng.uniform(0.04, 0.6, (n, 2))
    b = np.concatenate([np.clip(c - s / 2, 0., 1.), np.clip(c + s / 2, 0., 1.)], 1)
    return b.astype(np.float32)


def _grid512():
    """G = 512 full: a 16 x 32 grid of small boxes"""
    y, x = np.meshgrid(np.arange(16), np.arange(32), indexing='ij')
    y0, x0 = (y.reshape(-1) + 0.1) / 16., (x.reshape(-1) + 0.1) / 32.
    return np.stack([y0, x0, y0 + 0.8 / 16., x0 + 0.8 / 32.], 1).astype(np.float32)


def box_sets():
    rng = np.random.default_rng(5)
    eight = _mixed(rng, 8)
    return [
        ('large', np.array([5], np.int32), np.array([[0.05, 0.05, 0.95, 0.95]], np.float32)),
        ('tiny', np.array([3], np.int32), np.array([[0.50, 0.50, 0.52, 0.53]], np.float32)),
        ('eight', np.arange(1, 9, dtype=np.int32), eight),
        ('none', np.zeros(0, np.int32), np.zeros((0, 4), np.float32)),
        ('label0', np.array([0, 4, 0, 9], np.int32), _mixed(rng, 4)),
        ('full512', (np.arange(512) % 20 + 1).astype(np.int32), _grid512()),
    ]


def cases():
    """every shape with every box set, the seed walking through SEEDS; then every box set once more on a VOC shape with
    each remaining seed"""
    out = []
    sets = box_sets()
    k = 0
    for si, shape in enumerate(SHAPES):
        img = rand_image(*shape, seed=si)
        for name, labels, boxes in sets:
            out.append(('%dx%d-%s-s%d' % (shape + (name, SEEDS[k % 4])), img, labels, boxes, SEEDS[k % 4], 100 + k))
            k += 1
    img = rand_image(375, 500, seed=99)
    for name, labels, boxes in sets:
        for seed in SEEDS:
            out.append(('375x500-%s-s%d-b' % (name, seed), img, labels, boxes, seed, 100 + k))
            k += 1
    # a 5-row image and a box whose centre lies in one pixel row: the patch of height int32((4/5 - 3/5) * 5) = 0
    out.append(('5x6-one-row-s26', rand_image(5, 6, seed=3), np.array([2], np.int32),
                np.array([[0.62, 0.1, 0.78, 0.9]], np.float32), 26, 7))
    return out
