"""Overlays restated in numpy, the definition of DESIGN.md "Overlays": region, outline, discs, label, colour, list, ownership, value and
pixel counts.  fp32 with one rounding per operation where it is floating point (np.float32 scalars never contract), integers
otherwise.  Brute force on purpose: every primitive is evaluated at every pixel of the frame, and a pixel goes to the first region of
the list that covers it.  The native code is compared with this byte for byte."""
import numpy as np

f32 = np.float32
LABEL_NONE, LABEL_SCORE, LABEL_ID = 0, 1, 2
MAX_REGIONS = 1024
PALETTE = ((0, 0, 255), (0, 255, 0), (255, 0, 0), (0, 255, 255), (255, 0, 255), (255, 255, 0), (0, 128, 255), (255, 128, 0))
# 5 x 7, rows top to bottom, the most significant of the five bits on the left
GLYPHS = {
    0: (0x0E, 0x11, 0x13, 0x15, 0x19, 0x11, 0x0E),
    1: (0x04, 0x0C, 0x04, 0x04, 0x04, 0x04, 0x0E),
    2: (0x0E, 0x11, 0x01, 0x02, 0x04, 0x08, 0x1F),
    3: (0x1F, 0x02, 0x04, 0x02, 0x01, 0x11, 0x0E),
    4: (0x02, 0x06, 0x0A, 0x12, 0x1F, 0x02, 0x02),
    5: (0x1F, 0x10, 0x1E, 0x01, 0x01, 0x11, 0x0E),
    6: (0x06, 0x08, 0x10, 0x1E, 0x11, 0x11, 0x0E),
    7: (0x1F, 0x01, 0x02, 0x04, 0x08, 0x08, 0x08),
    8: (0x0E, 0x11, 0x11, 0x0E, 0x11, 0x11, 0x0E),
    9: (0x0E, 0x11, 0x11, 0x0F, 0x01, 0x02, 0x0C),
}


class Spec:
    """a resolved rf_overlay_spec: 0 = the default, as in the header"""

    def __init__(self, thickness=0, radius=0, box=(0, 0, 0), point=(0, 0, 0), text=(0, 0, 0), colors_set=False, alpha=0, label=0,
                 font_scale=0, color_by_id=False, max_regions=0, coast=0, default_regions=256):
        self.t = int(thickness) or 2
        self.r = -1 if int(radius) < 0 else (int(radius) or 2)
        pick = lambda c, d: tuple(int(v) for v in c) if (colors_set or any(c)) else d      # noqa: E731
        self.box, self.point, self.text = pick(box, (0, 0, 255)), pick(point, (0, 255, 0)), pick(text, (255, 255, 255))
        self.a = int(alpha) or 255
        self.label = int(label)
        self.f = int(font_scale) or 2
        self.color_by_id = bool(color_by_id)
        self.max_regions = int(max_regions) or min(int(default_regions), MAX_REGIONS)
        self.coast = int(coast)

    def coast_limit(self, max_missed):
        return max_missed if self.coast == 0 else (0 if self.coast < 0 else self.coast)


def _clamp(e):
    return f32(-4096) if e < f32(-4096) else (f32(8192) if e > f32(8192) else e)


class Region:
    """one entry of the list: the floored box, the disc centres that exist, the label's digits, the colour, whether it coasts"""

    def __init__(self, spec, face, scale=1.0, track_id=0, coasting=False):
        face = np.asarray(face, f32).reshape(15)
        self.valid, self.coasting, self.centres, self.digits = False, bool(coasting), [], []
        with np.errstate(all="ignore"):
            s = f32(scale)
            bx1, by1, bx2, by2 = (f32(v * s) for v in face[1:5])
            w, h = f32(bx2 - bx1), f32(by2 - by1)
            if not all(np.isfinite(v) for v in (bx1, by1, bx2, by2, w, h)) or not (w >= 0 and h >= 0):
                return
            self.valid = True
            self.x0, self.y0, self.x1, self.y1 = (int(np.floor(_clamp(v))) for v in (bx1, by1, bx2, by2))
            if not coasting and spec.r >= 0:
                for k in range(5):
                    px, py = f32(face[5 + k] * s), f32(face[10 + k] * s)
                    if np.isfinite(px) and np.isfinite(py):
                        self.centres.append((int(np.floor(_clamp(px))), int(np.floor(_clamp(py)))))
            track_id = int(track_id)
            self.colour = PALETTE[track_id & 7] if spec.color_by_id and track_id > 0 else spec.box
            if spec.label == LABEL_SCORE:
                p = f32(face[0] * f32(100))
                v = 0 if np.isnan(p) else int(min(max(p, f32(0)), f32(99)))
                self.digits = [v // 10, v % 10]
            elif spec.label == LABEL_ID and track_id > 0:
                self.digits = [int(c) for c in str(track_id % 1000000)]


def primitives(spec, r, rows, cols):
    """(covered, colour): which pixels of a rows x cols frame region r paints and with what, priority glyph > plate > disc (lower k
    first) > outline.  Every primitive is evaluated over the whole frame."""
    covered = np.zeros((rows, cols), bool)
    colour = np.zeros((rows, cols, 3), np.uint8)
    if not r.valid:
        return covered, colour
    y, x = np.mgrid[0:rows, 0:cols]
    t, o = spec.t, spec.t // 2
    ox0, oy0, ox1, oy1 = r.x0 - o, r.y0 - o, r.x1 + o, r.y1 + o
    outline = (x >= ox0) & (x <= ox1) & (y >= oy0) & (y <= oy1)
    outline &= ~((x >= ox0 + t) & (x <= ox1 - t) & (y >= oy0 + t) & (y <= oy1 - t))
    if r.coasting:
        outline &= (((x - ox0) + (y - oy0)) // (2 * t)) % 2 == 0
    covered |= outline
    colour[outline] = r.colour
    for cx, cy in reversed(r.centres):                                       # the lowest k is painted last: it ends on top
        disc = (x - cx) ** 2 + (y - cy) ** 2 <= spec.r ** 2
        covered |= disc
        colour[disc] = spec.point
    n, f = len(r.digits), spec.f
    if n:
        pw, ph = f + 6 * f * n, 9 * f
        top = oy0 - ph if oy0 - ph >= 0 else oy0
        plate = (x >= ox0) & (x < ox0 + pw) & (y >= top) & (y < top + ph)
        covered |= plate
        colour[plate] = r.colour
        # glyph bit (gx, gy) of digit j covers the f x f square at plate-relative (f + 6 f j + f gx, f + f gy)
        bits = np.array([[[(GLYPHS[d][gy] >> (4 - gx)) & 1 for gx in range(5)] + [0] for gy in range(7)] for d in r.digits], bool)
        u, v = x - ox0 - f, y - top - f
        inside = plate & (u >= 0) & (v >= 0) & (v < 7 * f)
        j, gx, gy = np.where(inside, u // (6 * f), 0), np.where(inside, (u % (6 * f)) // f, 5), np.where(inside, v // f, 0)
        colour[inside & bits[j, gy, gx]] = spec.text
    return covered, colour


def draw(spec, frame, regions):
    """(annotated copy of `frame`, pixels each region painted) for a region list already cut at max_regions"""
    out = frame.copy()
    rows, cols = frame.shape[:2]
    taken = np.zeros((rows, cols), bool)
    pixels = np.zeros(len(regions), np.int32)
    a = spec.a
    for q, r in enumerate(regions):
        covered, colour = primitives(spec, r, rows, cols)
        mine = covered & ~taken
        taken |= covered
        pixels[q] = int(mine.sum())
        if pixels[q]:
            out[mine] = ((frame[mine].astype(np.int64) * (255 - a) + colour[mine].astype(np.int64) * a + 127) // 255).astype(np.uint8)
    return out, pixels


def coasting_tracks(table, limit):
    """(face, id) of a track_ref table's live tracks with 1 <= missed <= limit, ascending slot order, at `last` (of a motion tracker:
    pass motion_ref.predicted_table(), whose `last` faces are the predicted ones)"""
    return [(np.frombuffer(t["last"].tobytes(), f32), int(t["id"])) for t in table if t["id"] != 0 and 1 <= t["missed"] <= limit]


def region_list(spec, faces, scale, ids=None, table=None, max_missed=0):
    """(regions cut at max_regions, true length) of one image: redaction's list -- faces in score order, then the coasting tracks"""
    faces = np.asarray(faces)
    rows15 = (np.ascontiguousarray(faces).view(f32) if faces.dtype.names else faces.astype(f32)).reshape(-1, 15)
    entries = [(f, scale, int(ids[k]) if ids is not None and k < len(ids) else 0, False) for k, f in enumerate(rows15)]
    if table is not None:
        entries += [(f, 1.0, i, True) for f, i in coasting_tracks(table, spec.coast_limit(max_missed))]
    return [Region(spec, f, s, i, c) for f, s, i, c in entries[:spec.max_regions]], len(entries)


def overlay_image(spec, frame, faces, scale=1.0, ids=None, table=None, max_missed=0):
    """(annotated copy, pixels padded to max_regions, true region count); a None / empty frame has no regions"""
    if frame is None or frame.size == 0:
        return frame, np.zeros(spec.max_regions, np.int32), 0
    regions, true = region_list(spec, faces, scale, ids, table, max_missed)
    out, px = draw(spec, frame, regions)
    pixels = np.zeros(spec.max_regions, np.int32)
    pixels[:len(px)] = px
    return out, pixels, true
