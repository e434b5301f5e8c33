"""Readers of the split-precision planes layout (include/xdet.h, xdet_split_f32) shared by the op-level GPU tests."""
import numpy as np


def planes_raw(buf, n_pix, ld):
    """one f16 plane [ceil(n_pix/16)][ld/32][16][32] -> its raw halves as uint16 [ceil(n_pix/16)*16][ld] (pixel-major)"""
    from xdet.runtime import to_host
    g = -(-n_pix // 16)
    return to_host(buf.ptr, (g, ld // 32, 16, 32), np.uint16).transpose(0, 2, 1, 3).reshape(g * 16, ld)


def planes_to_f32(hi_buf, lo_buf, n_pix, ld):
    """[pix/16][ld/32][16][32] f16 hi / lo planes -> f32 [n_pix][ld] of hi + lo"""
    hi = planes_raw(hi_buf, n_pix, ld).view(np.float16).astype(np.float32)
    lo = planes_raw(lo_buf, n_pix, ld).view(np.float16).astype(np.float32)
    return (hi + lo)[:n_pix]
