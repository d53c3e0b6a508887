"""numpy restatement of change regions ("Change regions"): a helper, not a test.

A stream keeps one int32 per block of the frame (the reference) and a frame counter.  The value of a block is S = the sum of
29 b + 150 g + 77 r over its pixels inside the frame.  The first step seeds (ref = S, nothing changed); every other step marks a block
when |S - ref| > 16 * thr_q4 * npix and then moves the reference by (S - ref) >> adapt_shift (floors).  The mask, dilated by one block
unless that is off, falls into 8-connected components (label = smallest raster index, count, bounding box); those with
count >= min_blocks are ordered by count descending, label ascending, the first max_regions kept; a kept component's pixel rectangle
goes through roi_ref.from_faces (coord scale 1) and roi_ref.plan_one.  Slots behind `kept`, and every slot of a seeding step, are the
void record.  retinaface_amd/csrc/change.h, the two kernels (kernels.hip change_blocks_kernel / change_regions_kernel) and the entry
points rf_change_step_host / rf_change_regions_device / rf_detect_change_roi_batch* are checked byte for byte against this file.
"""
import numpy as np

import roi_ref as rr

VOID = 2
VOID_CELL = (0, 0, 0, 0, 0, 0, 0, VOID)
MAX_BLOCKS = 16384


def resolve(block=0, thr_q4=0, adapt_shift=0, dilate=0, min_blocks=0, max_regions=0):
    """the spec with its defaults: (B, thr_q4, a, dilate on, min_blocks, R)"""
    return block or 16, thr_q4 or 128, adapt_shift, dilate != 2, min_blocks or 2, max_regions or 16


def grid_of(rows, cols, B):
    return -(-cols // B), -(-rows // B)


def block_sums(frame, B):
    """(S, npix), each (bh, bw): int64 sums and pixel counts"""
    rows, cols = frame.shape[:2]
    bw, bh = grid_of(rows, cols, B)
    y = frame[:, :, 0].astype(np.int64) * 29 + frame[:, :, 1].astype(np.int64) * 150 + frame[:, :, 2].astype(np.int64) * 77
    pad = np.zeros((bh * B, bw * B), np.int64)
    pad[:rows, :cols] = y
    ones = np.zeros((bh * B, bw * B), np.int64)
    ones[:rows, :cols] = 1
    return pad.reshape(bh, B, bw, B).sum((1, 3)), ones.reshape(bh, B, bw, B).sum((1, 3))


def dilate_mask(mask):
    bh, bw = mask.shape
    pad = np.zeros((bh + 2, bw + 2), bool)
    pad[1:-1, 1:-1] = mask != 0
    out = np.zeros((bh, bw), bool)
    for dy in range(3):
        for dx in range(3):
            out |= pad[dy:dy + bh, dx:dx + bw]
    return out


def components(marked):
    """[(label, count, bx0, by0, bx1, by1)] of the 8-connected sets of a (bh, bw) bool array, by union-find"""
    bh, bw = marked.shape
    parent = {}

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for y in range(bh):
        for x in range(bw):
            if not marked[y, x]:
                continue
            i = y * bw + x
            parent[i] = i
            for dy, dx in ((0, -1), (-1, -1), (-1, 0), (-1, 1)):
                yy, xx = y + dy, x + dx
                if 0 <= yy and 0 <= xx < bw and marked[yy, xx]:
                    a, b = find(i), find(yy * bw + xx)
                    if a != b:
                        parent[max(a, b)] = min(a, b)
    comps = {}
    for i in parent:
        r = find(i)                                     # the root is the smallest index: unions always keep the smaller
        y, x = divmod(i, bw)
        c = comps.setdefault(r, [r, 0, x, y, x, y])
        c[1] += 1
        c[2], c[3], c[4], c[5] = min(c[2], x), min(c[3], y), max(c[4], x), max(c[5], y)
    return [tuple(comps[r]) for r in sorted(comps)]


def select(comps, min_blocks, R):
    return sorted((c for c in comps if c[1] >= min_blocks), key=lambda c: (-c[1], c[0]))[:R]


def region_cell(comp, B, rows, cols, margin_q8, cw, ch, max_zoom=0):
    """(region (x, y, w, h), the 8 ints of the cell) of a kept component"""
    _, _, bx0, by0, bx1, by1 = comp
    face = np.zeros(15, np.float32)
    face[1:5] = bx0 * B, by0 * B, min(cols, (bx1 + 1) * B), min(rows, (by1 + 1) * B)
    rois = rr.from_faces(face.reshape(1, 15), 1.0, margin_q8)
    if not rois:
        return (0, 0, 0, 0), VOID_CELL
    r = tuple(int(v) for v in rois[0])
    return r, r + rr.plan_one(r, cw, ch, max_zoom)


class Stream:
    """the state of one stream"""

    def __init__(self, rows, cols, **spec):
        self.rows, self.cols = rows, cols
        self.B, self.thr, self.a, self.dilate, self.min_blocks, self.R = resolve(**spec)
        self.bw, self.bh = grid_of(rows, cols, self.B)
        assert self.bw * self.bh <= MAX_BLOCKS
        self.reset()

    def reset(self):
        self.ref = np.zeros((self.bh, self.bw), np.int32)
        self.mask = np.zeros((self.bh, self.bw), np.uint8)
        self.frames = 0

    def step(self, frame, margin_q8, view_w, view_h, grid=0, max_zoom=0):
        """one step: (mask (bh, bw) uint8 before dilation, regions (R, 4), cells (R, 8), info (4,)), all int32 but the mask"""
        assert frame.shape[:2] == (self.rows, self.cols)
        g = rr.resolve(grid)[0]
        assert view_w % g == 0 and view_h % g == 0 and (view_w // g) % 4 == 0
        S, npix = block_sums(frame, self.B)
        regions = np.zeros((self.R, 4), np.int32)
        cells = np.array([VOID_CELL] * self.R, np.int32).reshape(self.R, 8)
        seed = self.frames == 0
        self.frames += 1
        if seed:
            self.ref = S.astype(np.int32)
            self.mask = np.zeros((self.bh, self.bw), np.uint8)
            return self.mask.copy(), regions, cells, np.array([0, 0, 0, 1], np.int32)
        d = S - self.ref.astype(np.int64)
        self.mask = (np.abs(d) > 16 * self.thr * npix).astype(np.uint8)
        self.ref = (self.ref.astype(np.int64) + (d >> self.a)).astype(np.int32)      # >> on int64 floors
        changed = int(self.mask.sum())
        comps, kept = [], []
        if changed:
            comps = components(dilate_mask(self.mask) if self.dilate else self.mask != 0)
            kept = select(comps, self.min_blocks, self.R)
        for k, c in enumerate(kept):
            regions[k], cells[k] = region_cell(c, self.B, self.rows, self.cols, margin_q8, view_w // g, view_h // g, max_zoom)
        return self.mask.copy(), regions, cells, np.array([changed, len(comps), len(kept), 0], np.int32)


def mask_frames(rows, cols, B, mask):
    """(seed, frame): a zero frame and a frame with 255 in the blocks of `mask` ((bh, bw)), the rest zero"""
    seed = np.zeros((rows, cols, 3), np.uint8)
    frame = seed.copy()
    for by, bx in zip(*np.nonzero(np.asarray(mask))):
        frame[by * B:(by + 1) * B, bx * B:(bx + 1) * B] = 255
    return seed, frame
