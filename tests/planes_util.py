"""Readers of the split-precision planes layout (include/xdet.h, xdet_split_f32) shared by the op-level GPU tests."""
import numpy as np


def planes_rows(flat, n_pix, ld):
    """the halves of one plane [ceil(n_pix/16)][ld/32][16][32], already on the host, as [ceil(n_pix/16)*16][ld] (pixel-major;
    a view where `flat` allows it; whatever lies behind the plane is left out)"""
    g = -(-n_pix // 16)
    return np.asarray(flat)[:g * 16 * ld].reshape(g, ld // 32, 16, 32).transpose(0, 2, 1, 3).reshape(g * 16, ld)


def planes_raw(buf, n_pix, ld):
    """one f16 plane [ceil(n_pix/16)][ld/32][16][32] -> its raw halves as uint16 [ceil(n_pix/16)*16][ld] (pixel-major)"""
    from xdet.runtime import to_host
    return planes_rows(to_host(buf.ptr, (-(-n_pix // 16) * 16 * ld,), np.uint16), n_pix, ld)


def planes_to_f32(hi_buf, lo_buf, n_pix, ld):
    """[pix/16][ld/32][16][32] f16 hi / lo planes -> f32 [n_pix][ld] of hi + lo"""
    hi = planes_raw(hi_buf, n_pix, ld).view(np.float16).astype(np.float32)
    lo = planes_raw(lo_buf, n_pix, ld).view(np.float16).astype(np.float32)
    return (hi + lo)[:n_pix]
