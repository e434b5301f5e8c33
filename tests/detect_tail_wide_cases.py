"""Inputs of tests/test_gpu_detect_tail_wide.py: the detection tail beyond 1024 ROIs per image (csrc/detect.hip
bboxes_eval_wide_kernel).  Built on detect_tail_cases.banded(R, V), which takes any R and V: class c has exactly V[c - 1] valid
ROIs, rows 0 .. V - 1, with scores in exact ties of hundreds of ROIs.  tests/test_detect_tail_wide_math.py proves on the CPU
that each case has the property it is named for.

Every builder returns read-only arrays and caches them: the tests share one copy."""
import numpy as np

import detect_tail_cases as T

f32 = np.float32

# valid ROIs per class: 0, 1, 2; 2 * nms_topk +- 1 (nms_topk = 200); 512 | 513 (rank counting | sort); 1024 | 1025 (a sort of
# 1024 | 2048 slots, and the narrow form's last R); 1088 = 17 * 64; 1536; R
V_1800 = [0, 1, 2, 399, 400, 401, 511, 512, 513, 1023, 1024, 1025, 1087, 1088, 1089, 1535, 1536, 1537, 1799, 1800]
# R = 2049: the first R with 4096 key slots; V 2047 | 2048 | 2049: a sort of 2048 | 4096 slots
V_2049 = [0, 1, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049]
# R = 6144, the bound: 8192 key slots; V 4096 | 4097: a sort of 4096 | 8192 slots
V_6144 = [1, 513, 1025, 4095, 4096, 4097, 6143, 6144]
# no row >= 1024 is valid: the first 1024 rows alone give the same detections
V_PREFIX = [0, 1, 513, 1023, 1024]

CASES = {'r1800': (1800, V_1800), 'r2049': (2049, V_2049), 'r6144': (6144, V_6144), 'prefix': (1800, V_PREFIX)}
# (nms_threshold, nms_topk): the cut at 2 * nms_topk lies inside exact ties that span rows 1024 and 2048
SETTINGS = [(0.3, 200), (1.0, 256), (0.0, 3), (0.3, 1)]

_cache = {}


def case(name, flipped=False):
    """-> (logits [R, len(V) + 1], boxes [R, 4], V).  flipped: both reversed along the ROI axis -- the valid band of class c is
    then the LAST V[c - 1] rows, so every winner of a class with V <= R - 1024 lies at r >= 1024"""
    key = (name, flipped)
    if key not in _cache:
        R, V = CASES[name]
        logits, boxes = T.banded(R, V)
        if flipped:
            logits, boxes = np.ascontiguousarray(logits[::-1]), np.ascontiguousarray(boxes[::-1])
            logits.setflags(write=False)
            boxes.setflags(write=False)
        _cache[key] = (logits, boxes, list(V))
    return _cache[key]


def order_of(scores):
    """the tail's order of one class: ROI indices by descending score, ties to the lower index -- the order of the packed keys
    (score bits << 32) | (0xFFFFFFFF - r) for positive float32 scores, whose bits order as their values do"""
    s = np.asarray(scores, f32)
    assert (s >= 0).all()
    key = (s.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.arange(s.size, dtype=np.uint64))
    return np.argsort(key, kind='stable')[::-1]
