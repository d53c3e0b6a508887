"""numpy restatement of tracked region detection ("Tracked region detection"): a helper, not a test.

The regions of a frame are planned from a tracker's table.  Slot = region: region r of an image is slot r of the image's stream, so
every live tracked image has passes_of(max_tracks, grid) passes whatever the table holds.  A free slot, or a box roi_ref.from_faces
skips, gets the VOID record (every field zero, flags VOID): its cell is zero pixels and drops every face whose centre falls in it.  A
live slot's box is its track's `last` box, for a tracker with motion the box motion_ref.step matches against (motion_ref.predict, one
frame ahead); its region is roi_ref.from_faces' at coord scale 1, its cell roi_ref.plan_one's.  After roi_ref's face rule and merge one
frame step (track_ref.step / motion_ref.step) runs over the merged faces in merge order at coord scale 1.  The kernels
(retinaface_amd/csrc/kernels.hip roi_track_cells_kernel, roi_atlas_kernel), retinaface_amd/csrc/roi.h roi_track_cell and the entry
points rf_roi_cells_from_tracks / rf_roi_track_cells_device / rf_detect_track_roi_batch* are checked byte for byte against this file.
"""
import numpy as np

import motion_ref as mr
import roi_ref as rr
import track_ref as tr

VOID = 2
VOID_CELL = (0, 0, 0, 0, 0, 0, 0, VOID)


def track_cell(track, rec, mspec, margin_q8, cw, ch, max_zoom=0):
    """the 8 ints (x, y, w, h, level, x0, y0, flags) of one slot: track a TRACK record, rec its MOTION record or None"""
    if track["id"] == 0:
        return VOID_CELL
    if rec is None:
        row = np.frombuffer(np.asarray(track["last"]).tobytes(), np.float32)
    else:
        row = mr.predict(track, rec, 1, mspec)
    rois = rr.from_faces(row.reshape(1, 15), 1.0, margin_q8)
    if not rois:
        return VOID_CELL
    return tuple(int(v) for v in rois[0]) + rr.plan_one(rois[0], cw, ch, max_zoom)


def cells_of(table, motion, mspec, margin_q8, view_w, view_h, grid=0, max_zoom=0):
    """(max_tracks, 8) int32: the cells of a stream's table; motion None: a plain tracker"""
    g = rr.resolve(grid)[0]
    assert view_w % g == 0 and view_h % g == 0 and (view_w // g) % 4 == 0
    out = [track_cell(table[s], None if motion is None else motion[s], mspec, margin_q8, view_w // g, view_h // g, max_zoom) for s in range(len(table))]
    return np.array(out, np.int32).reshape(len(table), 8)


def stream_cells(stream, margin_q8, view_w, view_h, grid=0, max_zoom=0):
    """cells_of for a track_ref.Stream or a motion_ref.Stream"""
    has_motion = isinstance(stream, mr.Stream)
    return cells_of(stream.table, stream.motion if has_motion else None, stream.mspec if has_motion else None, margin_q8, view_w, view_h, grid, max_zoom)


def atlas(frame, cells, view_w, view_h, grid=0):
    """(passes, view_h, view_w, 3) uint8: the views of cell records; a void cell is zeros"""
    g = rr.resolve(grid)[0]
    cw, ch = view_w // g, view_h // g
    out = np.zeros((rr.passes_of(len(cells), g), view_h, view_w, 3), np.uint8)
    for r, c in enumerate(cells):
        if int(c[7]) & VOID:
            continue
        p, cell = divmod(r, g * g)
        cj, ci = divmod(cell, g)
        out[p, cj * ch:(cj + 1) * ch, ci * cw:(ci + 1) * cw] = rr.level_window(frame, int(c[4]), int(c[5]), int(c[6]), cw, ch)
    return out


def map_face(face, cells, p, view_w, view_h, grid=0):
    """roi_ref.map_face with the void drop: a face whose centre falls in a void cell is dropped"""
    g = rr.resolve(grid)[0]
    cw, ch = view_w // g, view_h // g
    f = np.asarray(face, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        cx, cy = (f[1] + f[3]) * rr.f32(0.5), (f[2] + f[4]) * rr.f32(0.5)
        ci = sum(1 for k in range(1, g) if cx >= rr.f32(k * cw))
        cj = sum(1 for k in range(1, g) if cy >= rr.f32(k * ch))
    r = p * g * g + cj * g + ci
    if r < len(cells) and int(cells[r][7]) & VOID:
        return None
    return rr.map_face(face, cells, p, view_w, view_h, grid)


def merge(cells, passes, view_w, view_h, nms_threshold, max_det, grid=0, vote_on=False, max_faces=0):
    """roi_ref.merge over cell records: (faces (k, 15), count, votes (k,), src_roi (k,), candidates)"""
    assert len(passes) == rr.passes_of(len(cells), grid)
    out, gs = [], []
    for p, faces in enumerate(passes):
        faces = np.asarray(faces, np.float32).reshape(-1, 15)[:max_det]
        for j, f in enumerate(faces):
            m = map_face(f, cells, p, view_w, view_h, grid)
            if m is not None:
                out.append(m[0])
                gs.append(m[1] * max_det + j)
    cand = np.stack(out) if out else np.zeros((0, 15), np.float32)
    return rr.tta_ref.merge_candidates(cand, np.array(gs, np.int64), nms_threshold, max_det, vote_on, max_faces) + (len(cand),)


def step(stream, faces, max_faces):
    """the frame step of one image over its merged faces ((k, 15) rows in merge order): (tags, ended, overflow)"""
    fn = mr.step if isinstance(stream, mr.Stream) else tr.step
    return fn(stream, np.asarray(faces, np.float32).reshape(-1, 15), 1.0, None, min(max_faces, tr.MAX_FACES))
