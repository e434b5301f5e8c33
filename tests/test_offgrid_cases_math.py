"""The off-grid size tables (offgrid_cases.py) do what test_gpu_offgrid.py relies on: they cover every SAME-padding
case of both nets, stay off the sizes the other whole-net tests run, the oracle fills every proposal row and finds
detections at each of them, and the oracle's own stride-2 pool and projection are right at the map sides that occur."""
import itertools

import numpy as np
import pytest

import offgrid_cases as C


def test_chains_restate_the_sizes_the_suite_already_runs():
    assert C.xception_chain(480) == (480, 239, 237, 119, 60, 30)
    assert C.xception_chain(256) == (256, 127, 125, 63, 32, 16)
    assert C.xception_chain(800) == (800, 399, 397, 199, 100, 50)
    assert C.xception_chain(126)[2:] == (60, 30, 15, 8) and C.xception_chain(203)[2:] == (99, 50, 25, 13)
    # the three of them are ONE padding case
    assert {C.xception_parity_class(S) for S in C.TESTED_ON_GRID['detector']} == {(0, 1, 1, 0)}
    assert C.resnet_chain(480)[-1] == 15 and C.resnet_chain(96)[-1] == 3 and C.resnet_chain(160)[-1] == 5


def test_chains_are_the_oracles_own_shapes(oracle):
    """same_pad / VALID arithmetic of the oracle's convs and pool, op by op, at every size of both tables"""
    for S in C.DETECTOR_SIZES:
        c = C.xception_chain(S)
        assert c[1] == (S - 3) // 2 + 1 and c[2] == c[1] - 3 + 1            # VALID, k = 3, strides 2 and 1
        for i in (2, 3, 4):
            assert oracle.same_pad(c[i], 3, 2)[2] == oracle.same_pad(c[i], 1, 2)[2] == c[i + 1]
            assert oracle.same_pad(c[i], 3, 2)[:2] == ((1, 1) if c[i] % 2 else (0, 1))
    for S in C.TRUNK_SIZES:
        c = C.resnet_chain(S)
        assert c[1] == (S + 6 - 7) // 2 + 1                                 # fixed padding 3/3, k = 7
        assert oracle.same_pad(c[1], 3, 2)[2] == c[2]                       # the SAME max pool
        for i in (2, 3, 4):                                                 # fixed padding 1/1, k = 3; 1x1 shortcut
            assert (c[i] + 2 - 3) // 2 + 1 == (c[i] - 1) // 2 + 1 == c[i + 1]


def test_detector_table_covers_all_sixteen_parity_classes():
    assert C.DETECTOR_SIZES == tuple(range(64, 80)) + (126, 203)
    small = [C.xception_parity_class(S) for S in range(64, 80)]
    assert set(small) == set(itertools.product((0, 1), repeat=4)) and len(set(small)) == 16
    assert all(C.xception_chain(S)[-1] in (4, 5) for S in range(64, 80))
    assert C.xception_parity_class(126) == (0, 0, 0, 1) and C.xception_parity_class(203) == (1, 1, 0, 1)
    assert C.xception_chain(203)[-1] == 13
    assert set(C.BIT_EQUALITY_SIZES) == {S for S in range(64, 80) if S % 2 == 0} | {203}
    assert set(C.BIT_EQUALITY_SIZES) <= set(C.DETECTOR_SIZES)


def test_trunk_table_covers_both_parities_at_every_strided_stage_and_is_minimal():
    chains = [C.resnet_chain(S) for S in C.TRUNK_SIZES]
    for stage in range(5):
        assert {c[stage] % 2 for c in chains} == {0, 1}, stage
    assert {S % 2 for S in C.TRUNK_SIZES} == {0, 1}
    assert all(64 <= S <= 130 for S in C.TRUNK_SIZES)
    # no single size can do it, so two is the smallest set; and no pair starts lower
    def covers(sizes):
        return all({C.resnet_chain(S)[i] % 2 for S in sizes} == {0, 1} for i in range(5))
    cands = [S for S in range(64, 131) if S % 32]
    pairs = [p for p in itertools.combinations(cands, 2) if covers(p)]
    assert len(C.TRUNK_SIZES) == 2 and pairs[0] == C.TRUNK_SIZES
    assert C.TRUNK_GRAPH_SIZE in C.TRUNK_SIZES and C.TRUNK_GRAPH_SIZE % 2 == 1
    assert C.TRUNK_SINGLE_SIZE in C.TRUNK_SIZES


def test_sizes_are_off_the_grid_and_off_the_spectral_maps():
    """No size is one the other whole-net tests run, none ends on a map with a DFT instantiated (so large_sep='auto'
    takes the direct (15,1) / (1,15) GEMMs), and none is a multiple of 32 -- except 64, the smallest size the nets accept,
    which the detector table holds as the one representative of the parity class of 256, 480 and 800 at a 4-wide map."""
    for S in C.DETECTOR_SIZES:
        assert S not in C.TESTED_ON_GRID['detector']
        assert C.xception_chain(S)[-1] not in C.SPECTRAL_MAPS
    assert [S for S in C.DETECTOR_SIZES if S % 32 == 0] == [64]
    assert C.xception_parity_class(64) == (0, 1, 1, 0)
    for S in C.TRUNK_SIZES:
        assert S % 32 and S not in C.TESTED_ON_GRID['trunk']
    # the direct large-separable GEMMs: the 15-tap window is wider than every map of the table, and at the 5- and
    # 13-wide maps M = N * fmap^2 rows is no multiple of 16; fmap is S / 16 at none of the sizes but 64
    fmaps = {S: C.xception_chain(S)[-1] for S in C.DETECTOR_SIZES}
    assert set(fmaps.values()) == {4, 5, 8, 13}
    assert (C.N_IMAGES * 5 * 5) % 16 and (C.N_IMAGES * 13 * 13) % 16
    assert [S for S in C.DETECTOR_SIZES if fmaps[S] * 16 == S] == [64]


@pytest.fixture(scope='module')
def oracle_runs(oracle, lh_weights):
    from xdet import weights as W
    runs = {}
    for S in C.DETECTOR_SIZES:
        tr = {}
        ref = oracle.lighthead_forward(W.synthetic_images(C.N_IMAGES, S, seed=S), lh_weights, rpn_post_nms_top_n=C.P,
                                       trace=tr)
        runs[S] = (ref, tr)
    return runs


@pytest.mark.parametrize('S', C.DETECTOR_SIZES)
def test_oracle_fills_every_proposal_row_and_detects(S, oracle_runs):
    """The dense and head comparisons of the GPU test run over all P rows of every image: they must all be proposals the
    NMS kept, not rows of the zero padding / upsample tail, and the detection match must not be vacuous."""
    ref, tr = oracle_runs[S]
    f = C.xception_chain(S)[-1]
    assert tr['feat'].shape == (C.N_IMAGES, f, f, 490) and tr['mid'].shape == (C.N_IMAGES, f, f, 728)
    assert tr['objectness'].shape == (C.N_IMAGES, f * f * C.ANCHORS_PER_CELL)
    assert tr['proposals'].shape == (C.N_IMAGES, C.P, 4)
    for i in range(C.N_IMAGES):
        pt = tr['proposal_traces'][i]
        assert pt['n_keep'] == C.P, (S, i, pt['n_keep'])                     # no row of the upsample tail
        n_det = sum(int((ref[i][c][0] > 0.01).sum()) for c in ref[i])
        assert n_det >= 1, (S, i)


torch = pytest.importorskip('torch')
F = torch.nn.functional


def _nchw(x):
    return torch.from_numpy(np.ascontiguousarray(x.transpose(0, 3, 1, 2)))


@pytest.mark.parametrize('H', sorted(set(C.ORACLE_POOL_SIDES)))
def test_oracle_stride2_pool_and_projection_vs_torch(H, oracle):
    """the two strided ops of an entry-flow block at the map sides of the tables (W = H + 1: both paddings in one case)"""
    for S in C.DETECTOR_SIZES:
        assert all(side in C.ORACLE_POOL_SIDES for side in C.xception_chain(S)[2:5])
    rng = np.random.default_rng(H)
    x = rng.standard_normal((2, H, H + 1, 5)).astype(np.float32)
    y = oracle.max_pool_3x3_s2_same(x)
    pt, pb, ho = oracle.same_pad(H, 3, 2)
    pl, pr, wo = oracle.same_pad(H + 1, 3, 2)
    ref = F.max_pool2d(F.pad(_nchw(x), (pl, pr, pt, pb), value=float('-inf')), 3, 2).numpy().transpose(0, 2, 3, 1)
    assert y.shape == ref.shape == (2, ho, wo, 5) and ho == -(-H // 2)
    assert np.array_equal(y, ref)
    w = rng.standard_normal((1, 1, 5, 7)).astype(np.float32)
    z = oracle.conv2d(x, w, 2, 'SAME')
    refz = F.conv2d(_nchw(x), torch.from_numpy(np.ascontiguousarray(w.transpose(3, 2, 0, 1))), stride=2)
    refz = refz.numpy().transpose(0, 2, 3, 1)
    assert z.shape == refz.shape == (2, ho, wo, 7)
    assert np.abs(z - refz).max() < 1e-5
    assert np.array_equal(z, x[:, ::2, ::2, :].reshape(-1, 5).dot(w[0, 0]).reshape(z.shape))     # pixel (2i, 2j), no pad
