"""Image sizes off the 32-pixel grid for whole-net tests of LightHeadDetector and ResNet50Trunk: plain data and the
side of every map along each net (test_offgrid_cases_math.py proves what the tables cover, test_gpu_offgrid.py runs
them).

Xception body: the stem is two 3x3 VALID convs (stride 2, then 1); blocks 2, 3 and 4 each end in a 3x3 stride-2 SAME
max pool next to a 1x1 stride-2 SAME projection; everything behind block 4 keeps the map.  SAME at stride 2 pads a 3x3
window 0/1 on an even input and 1/1 on an odd one, so the parities of the three pooled inputs select the padding of
every strided op of the body.  All sizes the suite ran so far (256, 480, 800) give odd, odd, even."""

P = 50                      # proposals kept per image (rpn_post_nms_top_n) in the off-grid runs
N_IMAGES = 2                # W.synthetic_images(N_IMAGES, S, seed=S), max_batch = N_IMAGES
ANCHORS_PER_CELL = 22

# 64..79: every parity combination of (S, block 2 input, block 3 input, block 4 input), maps 4 or 5 wide.
# 126: chain 60, 30, 15, 8 (even, even, odd).  203: odd S, chain 99, 50, 25, 13 (odd, even, odd), fmap 13.
DETECTOR_SIZES = tuple(range(64, 80)) + (126, 203)

# graph replay / batch invariance / pool_sub bit equalities: the eight even sizes of 64..79 and 203
BIT_EQUALITY_SIZES = tuple(range(64, 80, 2)) + (203,)

# The trunk has five stride-2 ops in a row (7x7 conv, 3x3 max pool, first block of stages 2, 3 and 4), each halving
# with ceil.  Two sizes whose chains differ in parity at every one of the five inputs are the smallest possible set;
# (66, 95) is the first such pair in 64..130 without a multiple of 32: 66, 33, 17, 9, 5 and 95, 48, 24, 12, 6.
TRUNK_SIZES = (66, 95)
TRUNK_GRAPH_SIZE = 95       # graph replay == eager at one odd size
TRUNK_SINGLE_SIZE = 66      # N = 1 at one size

# map sides at which the oracle's stride-2 pool and projection are checked against torch-CPU
ORACLE_POOL_SIDES = tuple(range(29, 38)) + tuple(range(15, 20)) + (8, 9, 10) + (60, 30, 15) + (99, 50, 25)

TESTED_ON_GRID = {'detector': (256, 480, 800), 'trunk': (96, 160, 480)}    # what the other whole-net tests run
SPECTRAL_MAPS = (16, 30, 50)                                              # feature maps with a DFT instantiated


def ceil_half(n):
    return -(-n // 2)


def xception_chain(S):
    """sides of (image, block1_conv1, stem_out = block 2 input, block 3 input, block 4 input, fmap)"""
    c1 = (S - 3) // 2 + 1
    b2 = c1 - 2
    b3 = ceil_half(b2)
    b4 = ceil_half(b3)
    return (S, c1, b2, b3, b4, ceil_half(b4))


def xception_parity_class(S):
    """(S, block 2 input, block 3 input, block 4 input) mod 2: the SAME padding of every strided op of the body, and
    whether the stem's last image row and column lie under a window (odd S) or not (even S)"""
    c = xception_chain(S)
    return (S % 2, c[2] % 2, c[3] % 2, c[4] % 2)


def resnet_chain(S):
    """sides of (image, conv1, pool = stages 1-2 input, stage 3 input, stage 4 input, output); entries 0..4 are the
    inputs of the five stride-2 ops"""
    chain = [S]
    for _ in range(5):
        chain.append(ceil_half(chain[-1]))
    return tuple(chain)
