"""What the whole-net GPU tests share when they compare with the oracle: the error measure of the dense stages, the
set matching of detections and the one admissible cause of a differing proposal set."""
import numpy as np

TOL = 1e-3


def rel_err(a, b):
    return float(np.abs(a - b).max()) / max(1.0, float(np.abs(b).max()))


def match_detections(got, ref, tol=TOL):
    """set matching per class: every oracle detection needs a distinct GPU detection whose score
    and box agree within tol (two detections whose scores differ by float noise may legitimately
    swap places in the score-ordered output)."""
    total = matched = extra = 0
    for c in ref:
        gs, gb = got[c]
        rs, rb = ref[c]
        kg, kr = int((gs > 0).sum()), int((rs > 0).sum())
        assert np.all(gs[kg:] == 0) and np.all(gb[kg:] == 0)            # zero padding
        used = np.zeros(kg, bool)
        for j in range(kr):
            d = np.maximum(np.abs(gs[:kg] - rs[j]), np.abs(gb[:kg] - rb[j]).max(1)) if kg else np.array([])
            d = np.where(used, np.inf, d)
            if kg and d.min() < tol:
                used[int(d.argmin())] = True
                matched += 1
        total += kr
        extra += kg - int(used.sum())
    return total, matched, extra


def explain_proposal_mismatch(oracle, tr, gpu_props):
    """A proposal set may differ from the oracle's ONLY through an NMS decision that sits on the 0.7 threshold:
    a GPU-only box must have, among the oracle's proposals, a partner whose IoU with it is within 1e-5 of the
    threshold (the suppressor that won on one side and lost on the other).  Anything else is a real bug."""
    ref = tr['proposals'][0]
    d = np.abs(gpu_props[:, None, :] - ref[None, :, :]).max(-1)
    only_gpu = gpu_props[d.min(1) >= TOL]
    assert 0 < len(only_gpu) <= 3, len(only_gpu)
    for b in only_gpu:
        both = np.concatenate([b[None], ref])
        ious = np.array([oracle.iou_tf(both, 0, j) for j in range(1, len(both))])
        near = np.abs(ious - 0.7).min()
        print('  GPU-only proposal %s: closest oracle-side IoU to the 0.7 threshold: |IoU - 0.7| = %.2e' % (b, near))
        assert near < 1e-5, near
