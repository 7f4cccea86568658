"""numpy specification of lfvio_track_source_set (include/lfvio.h): a tracker call of the single route takes the SOURCE
image and fills level 0 of its pyramid through the resident map.  Nothing here is new arithmetic: level 0 is image_ref.to_gray of
project_ref.remap — the grey value of the pixel lfvio_remap_apply would have written, that of a zero pixel for an outside entry.
lf-vio_amd/csrc/tracksource_plan.h holds the per-call check and a host copy of one lane of k_remap_gray; tests/test_tracksource_plan.py
holds both to this file.

  call_check   None, or why a tracker call on a width x height image is refused while the setting is on
  level0       the grey W x H image of a source image through float maps
  lanes        how many lanes the launch has (whole workgroups of 256, a lane per 4 pixels)"""
import numpy as np

import image_ref as ir
import project_ref as pr

MIN_SIDE, MAX_SIDE = pr.MIN_SIDE, pr.MAX_SIDE
THREADS, RUN = 256, 4


def set_check(src_width, src_height):
    """True: lfvio_track_source_set refuses (remap_side_check)."""
    return not (MIN_SIDE <= src_width <= MAX_SIDE and MIN_SIDE <= src_height <= MAX_SIDE)


def call_check(source, resident, fmt, width, height):
    """source: None (off) or (src_width, src_height); resident: None (no map) or the resident map's (width, height); fmt: None (the
    format setting is off: mono8, rows contiguous) or (encoding, step).  None: accepted; otherwise which refusal."""
    if source is None:
        return None
    if resident is None:
        return "no resident map"
    if tuple(resident) != (width, height):
        return "another size"
    enc, step = (0, 0) if fmt is None else fmt
    return "format" if pr.apply_check(enc, step, source[0], source[1]) else None


def upload_bytes(source, fmt):
    enc, step = (0, 0) if fmt is None else fmt
    return source[1] * (step or source[0] * ir.BPP[enc])


def level0(src, map_x, map_y, src_width, src_height, encoding=0, step=0):
    """src: uint8, src_height rows of `step` bytes (0: src_width * bytes per pixel) -> [height, width] uint8."""
    out = pr.remap(src, map_x, map_y, src_width, src_height, encoding, step)
    return ir.to_gray(out, map_x.shape[1], encoding)


def lanes(pixels):
    n = -(-pixels // RUN)
    return -(-n // THREADS) * THREADS
