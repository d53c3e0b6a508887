"""Face redaction restated in numpy, the definition of DESIGN.md "Face redaction": region, mask, cells, ownership, pixel counts and the
coasting list.  fp32 with one rounding per operation where it is floating point (np.float32 scalars never contract), Python integers
otherwise.  The native code is compared with this byte for byte."""
import numpy as np

f32 = np.float32
PIXELATE, FILL = 0, 1
RECT, ELLIPSE = 0, 1
MAX_REGIONS = 1024


class Spec:
    """a resolved rf_redact_spec: 0 = the default, as in the header"""

    def __init__(self, mode=0, shape=0, cells=0, margin=0.0, fill=(0, 0, 0), max_regions=0, coast=0, default_regions=256):
        self.mode, self.shape = int(mode), int(shape)
        self.cells = int(cells) or 8
        m = f32(margin)
        self.margin = f32(0.2) if m == 0 else (f32(0) if m < 0 else m)
        self.fill = tuple(int(v) for v in fill)
        self.max_regions = int(max_regions) or min(int(default_regions), MAX_REGIONS)
        self.coast = int(coast)

    def coast_limit(self, max_missed):
        return max_missed if self.coast == 0 else (0 if self.coast < 0 else self.coast)


class Region:
    """ux0, uy0, ux1, uy1: the unclipped rectangle; cx0, cy0, cx1, cy1: its intersection with the frame; c: the cell edge"""

    def __init__(self, valid, u=(0, 0, 0, 0), clip=(0, 0, 0, 0), c=0):
        self.valid = bool(valid)
        self.ux0, self.uy0, self.ux1, self.uy1 = (int(v) for v in u)
        self.cx0, self.cy0, self.cx1, self.cy1 = (int(v) for v in clip)
        self.c = int(c)

    def as_row(self):
        return np.array([self.ux0, self.uy0, self.ux1, self.uy1, self.cx0, self.cy0, self.cx1, self.cy1, self.c], np.int32)

    def empty(self):
        return not self.valid or self.cx1 <= self.cx0 or self.cy1 <= self.cy0


def _clamp(e):
    return f32(-4096) if e < f32(-4096) else (f32(8192) if e > f32(8192) else e)


def region(spec, box, scale, rows, cols):
    """box: x1, y1, x2, y2 (float32)"""
    with np.errstate(all="ignore"):
        s = f32(scale)
        bx1, by1, bx2, by2 = (f32(v) * s for v in box)
        w, h = f32(bx2 - bx1), f32(by2 - by1)
        if not all(np.isfinite(v) for v in (bx1, by1, bx2, by2, w, h)) or not (w >= 0 and h >= 0):
            return Region(False)
        mw, mh = f32(spec.margin * w), f32(spec.margin * h)
        ex1, ex2 = _clamp(f32(bx1 - mw)), _clamp(f32(bx2 + mw))
        ey1, ey2 = _clamp(f32(by1 - mh)), _clamp(f32(by2 + mh))
    ux0, ux1 = int(np.floor(ex1)), int(np.floor(ex2)) + 1
    uy0, uy1 = int(np.floor(ey1)), int(np.floor(ey2)) + 1
    c = (max(ux1 - ux0, uy1 - uy0) + spec.cells - 1) // spec.cells
    return Region(True, (ux0, uy0, ux1, uy1), (max(ux0, 0), max(uy0, 0), min(ux1, cols), min(uy1, rows)), c)


def mask(spec, r):
    """boolean mask over the region's clipped rectangle (shape (cy1 - cy0, cx1 - cx0)); None when that is empty"""
    if r.empty():
        return None
    hh, ww = r.cy1 - r.cy0, r.cx1 - r.cx0
    if spec.shape == RECT:
        return np.ones((hh, ww), bool)
    W, H = r.ux1 - r.ux0, r.uy1 - r.uy0
    a = 2 * np.arange(r.cx0, r.cx1, dtype=np.int64) + 1 - (r.ux0 + r.ux1)
    b = 2 * np.arange(r.cy0, r.cy1, dtype=np.int64) + 1 - (r.uy0 + r.uy1)
    return (a * a * H * H)[None, :] + (b * b * W * W)[:, None] <= W * W * H * H


def cell_image(frame, r):
    """the pixelated clipped rectangle of region r: every pixel holds its cell's value, formed from `frame` (the original)"""
    out = np.zeros((r.cy1 - r.cy0, r.cx1 - r.cx0, 3), np.uint8)
    c = r.c
    for gy in range((r.uy1 - r.uy0 + c - 1) // c):
        y0, y1 = max(r.uy0 + gy * c, r.cy0), min(r.uy0 + (gy + 1) * c, r.cy1)
        if y1 <= y0:
            continue
        for gx in range((r.ux1 - r.ux0 + c - 1) // c):
            x0, x1 = max(r.ux0 + gx * c, r.cx0), min(r.ux0 + (gx + 1) * c, r.cx1)
            if x1 <= x0:
                continue
            n = (y1 - y0) * (x1 - x0)
            s = frame[y0:y1, x0:x1].reshape(-1, 3).astype(np.int64).sum(0)
            out[y0 - r.cy0:y1 - r.cy0, x0 - r.cx0:x1 - r.cx0] = ((s + n // 2) // n).astype(np.uint8)
    return out


def redact(spec, frame, regions):
    """(redacted copy of `frame`, pixels each region owns) for a region list already cut at max_regions"""
    out = frame.copy()
    owner = np.full(frame.shape[:2], -1, np.int32)
    pixels = np.zeros(len(regions), np.int32)
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
        value = np.broadcast_to(np.array(spec.fill, np.uint8), mine.shape + (3,)) if spec.mode == FILL else cell_image(frame, r)
        out[r.cy0:r.cy1, r.cx0:r.cx1][mine] = value[mine]
    return out, pixels


def coasting_boxes(table, limit):
    """the `last` boxes of a track_ref table's live tracks with 1 <= missed <= limit, ascending slot order"""
    return [(t["last"]["x1"], t["last"]["y1"], t["last"]["x2"], t["last"]["y2"]) for t in table
            if t["id"] != 0 and 1 <= t["missed"] <= limit]


def region_list(spec, faces, scale, rows, cols, table=None, max_missed=0):
    """(regions cut at max_regions, true length) of one image: faces (rows of 15 floats or records with x1..y2, in score order), then
    the coasting tracks of `table` (a track_ref table; scale 1)"""
    faces = np.asarray(faces)
    rows15 = np.ascontiguousarray(faces).view(f32) if faces.dtype.names else faces.astype(f32)
    boxes = [(tuple(f[1:5]), scale) for f in rows15.reshape(-1, 15)]
    if table is not None:
        boxes += [(b, 1.0) for b in coasting_boxes(table, spec.coast_limit(max_missed))]
    return [region(spec, b, s, rows, cols) for b, s in boxes[:spec.max_regions]], len(boxes)


def redact_image(spec, frame, faces, scale=1.0, table=None, max_missed=0):
    """(redacted copy, pixels padded to max_regions, true region count); a None / empty frame has no regions"""
    if frame is None or frame.size == 0:
        return frame, np.zeros(spec.max_regions, np.int32), 0
    regions, true = region_list(spec, faces, scale, frame.shape[0], frame.shape[1], table, max_missed)
    out, px = redact(spec, frame, regions)
    pixels = np.zeros(spec.max_regions, np.int32)
    pixels[:len(px)] = px
    return out, pixels, true
