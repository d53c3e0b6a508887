"""Blur redaction restated in numpy, the definition of DESIGN.md "Blur redaction".  Region, mask, list, ownership and pixel counts are
those of redact_ref (imported, not restated); only the value an owned pixel takes is new: the frame blurred with `blur` box passes per
axis of radius rho = min(c, 64), every pass a rounded mean in integers with the border replicated.  blur = 0 is redact_ref itself.  The
native code is compared with this byte for byte."""
import numpy as np

import redact_ref as rr
from redact_ref import ELLIPSE, FILL, MAX_REGIONS, PIXELATE, RECT, f32, mask, region, region_list  # noqa: F401  (re-exported)

MAX_RADIUS = 64


class Spec(rr.Spec):
    """a resolved rf_redact_spec with its blur byte"""

    def __init__(self, blur=0, **kw):
        super().__init__(**kw)
        self.blur = int(blur)
        assert 0 <= self.blur <= 3 and (self.blur == 0 or self.mode == PIXELATE)


def radius(r):
    return min(r.c, MAX_RADIUS)


def pass1d(a, rho, axis):
    """one pass of radius rho along `axis`: out[i] = (sum of a[clamp(i + d)] for d in [-rho, rho] + rho) // (2 rho + 1)"""
    n = 2 * rho + 1
    a = np.moveaxis(a, axis, 0)
    L = a.shape[0]
    cs = np.cumsum(a[np.clip(np.arange(-rho - 1, L + rho), 0, L - 1)].astype(np.int64), axis=0)
    return np.moveaxis(((cs[n:] - cs[:-n] + rho) // n).astype(np.uint8), 0, axis)


def blurred(frame, rho, passes):
    """B(frame, rho, passes): the passes along x on every row, then the passes along y on every column"""
    out = frame
    for _ in range(passes):
        out = pass1d(out, rho, 1)
    for _ in range(passes):
        out = pass1d(out, rho, 0)
    return out


def redact(spec, frame, regions):
    """(redacted copy of `frame`, pixels each region owns) for a region list already cut at max_regions"""
    if not spec.blur:
        return rr.redact(spec, frame, regions)
    out = frame.copy()
    owner = np.full(frame.shape[:2], -1, np.int32)
    pixels = np.zeros(len(regions), np.int32)
    cache = {}
    for q, r in enumerate(regions):
        m = mask(spec, r)
        if m is None:
            continue
        own = owner[r.cy0:r.cy1, r.cx0:r.cx1]
        mine = m & (own < 0)
        own[mine] = q
        pixels[q] = int(mine.sum())
        if not mine.any():
            continue
        rho = radius(r)
        if rho not in cache:
            cache[rho] = blurred(frame, rho, spec.blur)           # of the ORIGINAL frame
        out[r.cy0:r.cy1, r.cx0:r.cx1][mine] = cache[rho][r.cy0:r.cy1, r.cx0:r.cx1][mine]
    return out, pixels


def redact_image(spec, frame, faces, scale=1.0, table=None, max_missed=0):
    """(redacted copy, pixels padded to max_regions, true region count); a None / empty frame has no regions"""
    if frame is None or frame.size == 0:
        return frame, np.zeros(spec.max_regions, np.int32), 0
    regions, true = region_list(spec, faces, scale, frame.shape[0], frame.shape[1], table, max_missed)
    out, px = redact(spec, frame, regions)
    pixels = np.zeros(spec.max_regions, np.int32)
    pixels[:len(px)] = px
    return out, pixels, true
