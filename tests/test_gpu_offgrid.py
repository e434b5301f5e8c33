"""Both nets against the oracle at image sizes off the 32-pixel grid (offgrid_cases.py; what the tables cover is
proved by test_offgrid_cases_math.py).  256, 480 and 800 are ONE case of the SAME padding of the body's strided ops,
all even, all on a map with a spectral large-separable form; here every parity combination runs through the plan, with
odd image sides, 4- to 13-wide maps, large_sep='auto' on the direct (15,1) / (1,15) GEMMs and fmap != S / 16.

The dense stages are compared separately from the discrete ones: the proposal stage and the head run on the ORACLE's
tensors, so a keep/suppress decision on the NMS threshold cannot fail a dense check nor hide behind one."""
import time

import numpy as np
import pytest

import offgrid_cases as C
from oracle_compare import TOL, rel_err, match_detections, explain_proposal_mismatch

pytestmark = pytest.mark.gpu

STAGE_TOL = 1e-4            # the project's bar on every dense stage (test_gpu_e2e.py::test_dense_stages)
KEPT = ('stem_out', 'entry_x')


def build_detector(weights, S, precision, n=C.N_IMAGES, **kw):
    from xdet.model import LightHeadDetector
    from xdet.runtime import set_precision
    set_precision(precision)
    try:
        return LightHeadDetector(weights, image_size=S, max_batch=n, rpn_post_nms_top_n=C.P, **kw)
    finally:
        set_precision('f32')


def oracle_entry_stages(oracle, imgs, w):
    """the oracle's `stem_out` (block 2's input) and `entry_x` (block 4's output): xception_body's first lines, for naming
    the first stage whose error jumps when a dense check fails"""
    def conv_bn(x, name, bn, stride, padding):
        return oracle.batch_norm(oracle.conv2d(x, w[name + '/kernel'], stride, padding), w, bn, oracle.XC_EPS)
    x = np.transpose(imgs, (0, 2, 3, 1))
    x = oracle.relu(conv_bn(x, 'block1_conv1', 'block1_conv1_bn', 2, 'VALID'))
    x = stem_out = oracle.relu(conv_bn(x, 'block1_conv2', 'block1_conv2_bn', 1, 'VALID'))
    for b, first_relu in ((2, False), (3, True), (4, True)):
        res = conv_bn(x, 'conv2d_%d' % (b - 1), 'batch_normalization_%d' % (b - 1), 2, 'SAME')
        x = oracle._sep_bn(x, w, 'block%d_sepconv1' % b, pre_relu=first_relu)
        x = oracle._sep_bn(x, w, 'block%d_sepconv2' % b)
        x = oracle.max_pool_3x3_s2_same(x) + res
    return stem_out, x


class Case(object):
    """one size: the images, the oracle's run and trace, and per precision a detector that has run them (dense buffers
    copied to the host: later tests overwrite the device tensors)"""

    def __init__(self, S, oracle, weights):
        from xdet import weights as W
        self.S, self.oracle, self.weights = S, oracle, weights
        self.chain = C.xception_chain(S)
        self.fmap = self.chain[-1]
        self.imgs = W.synthetic_images(C.N_IMAGES, S, seed=S)
        self.tr = {}
        self.ref = oracle.lighthead_forward(self.imgs, weights, rpn_post_nms_top_n=C.P, trace=self.tr)
        self.runs = {}

    def run(self, precision):
        if precision not in self.runs:
            n, na = C.N_IMAGES, self.fmap * self.fmap * C.ANCHORS_PER_CELL
            t0 = time.time()
            det = build_detector(self.weights, self.S, precision, keep=KEPT)
            t1 = time.time()
            got = det.forward(self.imgs)
            t2 = time.time()
            print('S %d [%s]: build %.2f s, first forward %.2f s' % (self.S, precision, t1 - t0, t2 - t1))
            host = {k: det.buffer(k, n).numpy().copy() for k in KEPT + ('mid_x', 'out', 'rpn_out', 'feat')}
            host['objectness'] = det.flat('objectness', (n, na))
            host['rpn_boxes'] = det.flat('rpn_boxes', (n, na, 4))
            host['proposals'] = det.flat('proposals', (n, C.P, 4))
            self.runs[precision] = (det, got, host)
        return self.runs[precision]


@pytest.fixture(scope='module', params=C.DETECTOR_SIZES)
def case(request, oracle, lh_weights):
    return Case(request.param, oracle, lh_weights)


@pytest.mark.parametrize('precision', ['f32', 'f16x3'])
def test_dense_stages_against_the_oracle(case, precision):
    det, _, host = case.run(precision)
    tr, n, f = case.tr, C.N_IMAGES, case.fmap
    # the plan's shapes are the chain's
    assert host['stem_out'].shape == (n, case.chain[2], case.chain[2], 64)
    assert host['entry_x'].shape == host['mid_x'].shape == (n, f, f, 728)
    assert host['out'].shape == (n, f, f, 2048) and host['feat'].shape == (n, f, f, 490)
    assert host['rpn_out'].shape[:3] == (n, f, f) and host['rpn_out'].shape[3] >= 132
    assert tr['mid'].shape == (n, f, f, 728) and tr['objectness'].shape == (n, f * f * C.ANCHORS_PER_CELL)
    errs = [('mid', rel_err(np.maximum(host['mid_x'], 0), tr['mid'])),
            ('out', rel_err(host['out'], tr['out'])),
            ('rpn_cls', rel_err(host['rpn_out'][..., :44], tr['rpn_cls'])),
            ('rpn_box', rel_err(host['rpn_out'][..., 44:132], tr['rpn_box'])),
            ('feat', rel_err(host['feat'], tr['feat']))]
    absolute = [('objectness', float(np.abs(host['objectness'] - tr['objectness']).max())),
                ('rpn_boxes', float(np.abs(host['rpn_boxes'] - tr['rpn_boxes']).max()))]
    print('offgrid dense S %d [%s]: ' % (case.S, precision) + ' '.join('%s %.2e' % e for e in errs + absolute))
    if not all(e < STAGE_TOL for _, e in errs + absolute):
        # the first stage whose error jumps: the two kept tensors of the entry flow in front of the compared ones
        stem_out, entry_x = oracle_entry_stages(case.oracle, case.imgs, case.weights)
        front = [('stem_out', rel_err(host['stem_out'], stem_out)), ('entry_x', rel_err(host['entry_x'], entry_x))]
        print('offgrid dense S %d [%s] by stage: ' % (case.S, precision) + ' '.join('%s %.2e' % e for e in front + errs))
        chain = front + errs[:2]                             # stem_out -> entry_x -> mid -> out, in data-flow order
        jump = next((b[0] for a, b in zip([('image', 1e-7)] + chain, chain) if not b[1] < 10 * max(a[1], 1e-6)), None)
        first = next((name for name, e in front + errs + absolute if not e < STAGE_TOL), None)
        print('  first stage over the bar: %s; first stage whose error is 10x its input\'s: %s' % (first, jump))
    for name, e in errs + absolute:
        assert e < STAGE_TOL, (case.S, precision, name, e)


def test_discrete_stages_on_the_oracles_tensors(case):
    """get_proposals on the oracle's scores and boxes: the same proposals, exactly.  get_head on the oracle's feature map
    and proposals: PsRoiAlign samples 7 x 7 bins of boxes on a 4- to 13-wide map (every bin below one pixel at the small
    ones) -- logits and regressions within 2e-4."""
    from xdet import model as M
    det, _, _ = case.run('f16x3')
    tr = case.tr
    with det.scope():
        props = M.get_proposals(tr['objectness'], tr['rpn_boxes'], None, 5000, C.P, 0.7, 16. / 480, False,
                                'channels_first')
        assert props.shape == tr['proposals'].shape
        assert np.array_equal(props, tr['proposals']), (case.S, int((props != tr['proposals']).any(-1).sum()))
        c, r = M.get_head(tr['feat'], None, 7, 7, None, tr['proposals'], 21, False, False, 0, 'channels_first',
                          'final_head')
    e_cls, e_reg = float(np.abs(c - tr['cls']).max()), float(np.abs(r - tr['reg']).max())
    print('offgrid discrete S %d: cls %.2e reg %.2e' % (case.S, e_cls, e_reg))
    assert e_cls < 2e-4 and e_reg < 2e-4, (case.S, e_cls, e_reg)


def same_detections(a, b):
    return all(np.array_equal(a[i][c][0], b[i][c][0]) and np.array_equal(a[i][c][1], b[i][c][1])
               for i in range(len(a)) for c in a[i])


def test_whole_forward_detections(case):
    """the product arithmetic end to end, with the rule of test_other_baseline_configs: a proposal set may differ from the
    oracle's only by a decision within 1e-5 of the NMS threshold"""
    _, got, host = case.run('f16x3')
    tr, ref, oracle = case.tr, case.ref, case.oracle
    for i in range(C.N_IMAGES):
        props = host['proposals'][i]
        d = np.abs(props[:, None, :] - tr['proposals'][i][None, :, :]).max(-1)
        n_same = int((d.min(1) < TOL).sum())
        if n_same != C.P:
            print('S %d image %d: proposals with a match in the oracle set: %d / %d' % (case.S, i, n_same, C.P))
            explain_proposal_mismatch(oracle, {'proposals': tr['proposals'][i:i + 1]}, props)
        total, matched, extra = match_detections(got[i], ref[i])
        print('offgrid S %d image %d: oracle detections %d matched %d extra %d' % (case.S, i, total, matched, extra))
        assert total > 0
        if n_same == C.P:
            assert matched == total and extra == 0, (case.S, i, matched, total, extra)
        else:       # one flipped keep/suppress decision changes a handful of head inputs
            assert matched >= total - max(2, total // 50) and extra <= max(2, total // 50)


def test_split_pool_forms_equal_the_whole_pool(case):
    """Below 100 x 100 pixels the default plan pools blocks 2-4 with the whole 3x3 pass, which is every block at these sizes:
    pool='split_all' puts the horizontal half into the fused block's 15-window tiles and the vertical half, the add and
    (pool_sub) the next projection's subsampled planes into the pass behind it -- the forms the large maps of 480 and 800
    run, here at every padding parity.  max and one add per element in the same order: the same bits
    (test_gpu_hpool_tile_width.py and test_pool_pass_that_writes_the_next_projections_input claim so per op and at 480)."""
    _, eager, host = case.run('f16x3')
    for opts in (dict(pool='split_all'), dict(pool='split_all', pool_sub='off')):
        net = build_detector(case.weights, case.S, 'f16x3', keep=KEPT, **opts)
        got = net.forward(case.imgs)
        for k in KEPT + ('mid_x', 'out', 'feat'):
            a = net.buffer(k, C.N_IMAGES).numpy()
            bad = np.argwhere(a != host[k])
            assert np.array_equal(a, host[k]), (case.S, opts, k, len(bad), bad[:1].tolist())
        assert same_detections(got, eager), (case.S, opts)


def test_poisoned_workspace_changes_nothing(case):
    """workspace='poison' puts NaN bits behind every recycled f32 tensor in front of its producer.  Off the grid the pixel
    counts are multiples of neither the 16-pixel plane groups nor the GEMM tiles (2 x 25, 2 x 169 rows), so a consumer that
    rounds its reads up past the tensor would pick them up: the same bits as the default net, eager and by graph replay."""
    _, eager, host = case.run('f16x3')
    net = build_detector(case.weights, case.S, 'f16x3', workspace='poison')
    for graph in (False, True, True):
        got = net.forward(case.imgs, use_graph=graph)
        for k in ('mid_x', 'out', 'feat'):
            assert np.array_equal(net.buffer(k, C.N_IMAGES).numpy(), host[k]), (case.S, graph, k)
        assert same_detections(got, eager), (case.S, graph)


@pytest.mark.parametrize('S', C.BIT_EQUALITY_SIZES)
def test_bit_equalities(S, lh_weights):
    """no oracle: graph replay == eager; image 0 of a batch of 2 == a batch of 1 on the same max_batch = 2 net; the pool
    pass that writes the next projection's planes (pool_sub, default) == its own passes ('off')"""
    from xdet import weights as W
    imgs = W.synthetic_images(C.N_IMAGES, S, seed=S)
    names = ('mid_x', 'out', 'feat')
    det = build_detector(lh_weights, S, 'f16x3')
    eager = det.forward(imgs)
    bufs = {k: det.buffer(k, 2).numpy().copy() for k in names}
    for rep in range(2):                                     # capture, then replay
        assert same_detections(det.forward(imgs, use_graph=True), eager), (S, 'graph', rep)
    for k in names:
        assert np.array_equal(det.buffer(k, 2).numpy(), bufs[k]), (S, 'graph', k)
    one = det.forward(imgs[:1])
    assert same_detections(one, eager[:1]), (S, 'batch of 1')
    for k in names:
        assert np.array_equal(det.buffer(k, 1).numpy()[0], bufs[k][0]), (S, 'batch of 1', k)
    off = build_detector(lh_weights, S, 'f16x3', pool_sub='off')
    assert same_detections(off.forward(imgs), eager), (S, 'pool_sub')
    for k in names:
        assert np.array_equal(off.buffer(k, 2).numpy(), bufs[k]), (S, 'pool_sub', k)


# ---- the ResNet-50 v2 trunk ---------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def rn_weights():
    from xdet import weights as W
    return W.make_resnet50_weights(4321)


def build_trunk(w, S, precision, n):
    from xdet.resnet import ResNet50Trunk
    from xdet.runtime import set_precision
    set_precision(precision)
    try:
        return ResNet50Trunk(w, image_size=S, max_batch=n)
    finally:
        set_precision('f32')


@pytest.fixture(scope='module', params=C.TRUNK_SIZES)
def trunk_case(request, oracle, rn_weights):
    from xdet import weights as W
    S = request.param
    imgs = W.synthetic_images(C.N_IMAGES, S, seed=S)
    return S, imgs, oracle.resnet50_trunk(np.transpose(imgs, (0, 2, 3, 1)), rn_weights)


@pytest.mark.parametrize('precision', ['f32', 'f16x3'])
def test_trunk_against_the_oracle(trunk_case, rn_weights, precision):
    S, imgs, ref = trunk_case
    side = C.resnet_chain(S)[-1]
    net = build_trunk(rn_weights, S, precision, C.N_IMAGES)
    assert net.out_shape == (side, side, 2048)
    y = net.forward(imgs)
    assert y.shape == ref.shape == (C.N_IMAGES, side, side, 2048)
    err = rel_err(y, ref)
    print('offgrid trunk S %d [%s]: max error relative to the output scale %.2e' % (S, precision, err))
    assert err <= 1e-4, (S, precision, err)
    if S == C.TRUNK_SINGLE_SIZE:                             # N = 1 below max_batch, and on a net of its own
        assert np.array_equal(net.forward(imgs[:1])[0], y[0])
        y1 = build_trunk(rn_weights, S, precision, 1).forward(imgs[:1])
        assert rel_err(y1, ref[:1]) <= 1e-4


def test_trunk_graph_replay_is_the_eager_forward_at_an_odd_size(rn_weights):
    from xdet import weights as W
    from xdet.runtime import to_host
    S = C.TRUNK_GRAPH_SIZE
    net = build_trunk(rn_weights, S, 'f16x3', C.N_IMAGES)
    for seed in (1, 2):                                      # capture, then replay on new images
        imgs = W.synthetic_images(C.N_IMAGES, S, seed=seed)
        eager = net.forward(imgs)
        net.set_images(imgs)
        net.forward_device(C.N_IMAGES, use_graph=True)
        net.stream.synchronize()
        replay = to_host(net._out.ptr, (C.N_IMAGES,) + net.out_shape, np.float32)
        assert np.array_equal(eager, replay), (S, seed)
