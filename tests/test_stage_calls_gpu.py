"""The seven fused detect-and-post-process calls -- alignment, face batch (plain or gated), tracks, tracks + face batch, tracks + shots,
redaction / overlay, tracks + redaction / overlay -- share one stage-call skeleton in the engine: one open call with one image cursor,
one lane view, one lazy per-lane block.  Here they follow each other on ONE handle whose calls really split into launches of 8, 8, 8
and 1 images over three lanes (lane 0 is reused within the call, the last launch carries one image), with refused calls and the five
standalone calls in between, and every result must be the bytes the same call returns on a fresh handle with the same options -- which
test_gpu_align.py, test_face_batch_gpu.py, test_face_quality_gpu.py, test_track_gpu.py, test_shot_gpu.py, test_redact_gpu.py,
test_redact_blur_gpu.py and test_overlay_gpu.py pin to the numpy references."""
import numpy as np
import pytest

from test_gpu_align import rfa, rows_of, to_device  # noqa: F401  (rfa: fixture)
from test_pass_calls_gpu import frozen, handle
from test_tta_gpu import windows  # noqa: F401  (windows: fixture)

pytestmark = pytest.mark.gpu

N = 25                      # launches of 8, 8, 8 and 1
STREAMS = list(range(N))    # tracked steps: one image per stream


def fused(det, call, calls=1):
    """a fused call (or `calls` of them in a row) with its launches counted"""
    before = det.launch_stats()
    res = call()
    after = det.launch_stats()
    assert after["images"] - before["images"] == calls * N and after["launches"] - before["launches"] >= calls * 4, (before, after)
    return res


def test_stages_back_to_back_on_one_handle_equal_fresh_handles(rfa, windows, crop448):
    import torch
    seven = list(windows) + [crop448]
    dev = to_device(seven)
    ptrs, hw = [dev[i % 7].data_ptr() for i in range(N)], [448] * N
    args = (ptrs, hw, hw)

    def clones(which=range(N)):
        c = [dev[i % 7].clone() for i in which]
        torch.cuda.synchronize()
        return c

    def after(c):
        torch.cuda.synchronize()
        return [d.cpu().numpy() for d in c]

    def fresh(call, *a):
        ref = handle(rfa)
        try:
            return call(ref, *a)
        finally:
            ref.close()

    # a gate that rejects some faces and keeps some: the median sharpness of the faces the call considers
    quality = fresh(lambda det: det.detect_face_batch_device(*args, 0.5, crop_size=112, max_faces=8, host=False, return_quality=True)[4])
    sharp = np.concatenate([q["sharpness"] for q in quality])
    gate = dict(min_sharpness=float(np.median(sharp)))
    assert 0 < int((sharp < gate["min_sharpness"]).sum()) < len(sharp)

    def twice(det, trk, call):
        """a tracked step: a tracker made for the step, two calls in a row, so the second one sees live tracks"""
        try:
            return fused(det, lambda: (call(trk), call(trk)), calls=2)
        finally:
            trk.close()

    def aligned(det):
        return fused(det, lambda: det.detect_aligned_device(*args, 0.5, crop_size=112, max_faces=8))

    def batch(det):
        return fused(det, lambda: det.detect_face_batch_device(*args, 0.5, crop_size=112, dtype="f16", max_faces=8))

    def gated(det):
        return fused(det, lambda: det.detect_face_batch_device(*args, 0.5, crop_size=112, dtype="f16", max_faces=8, gate=gate, return_quality=True))

    def tracked(det):
        return twice(det, det.tracker(N), lambda t: det.detect_tracked_device(*args, t, STREAMS, 0.5))

    def tracked_batch(det):
        return twice(det, det.tracker(N), lambda t: det.detect_track_face_batch_device(*args, t, STREAMS, 0.5, crop_size=64, dtype="u8", max_faces=8,
                                                                                    gate=gate, return_quality=True))

    def shots(det):
        trk = det.tracker(N).enable_shots(crop_size=32, dtype="u8")
        return twice(det, trk, lambda t: (det.detect_track_shots_device(*args, t, STREAMS, 0.5, gate=gate, return_quality=True),
                                          [t.read_shots(s) for s in with_faces + [24]]))

    def redacting(spec, method="detect_redacted_device"):
        def step(det):
            c = clones()
            got = fused(det, lambda: getattr(det, method)([d.data_ptr() for d in c], hw, hw, 0.5, spec=spec))
            return got, det.last_pixels.copy(), after(c)
        return step

    def tracked_redacting(method, spec):
        def step(det):
            def call(t):
                c = clones()
                got = getattr(t, method)([d.data_ptr() for d in c], hw, hw, STREAMS, 0.5, spec=spec)
                return got, t.last_pixels.copy(), t.last_region_counts.copy(), after(c)
            return twice(det, det.tracker(N), call)
        return step

    steps = (("align", aligned), ("face batch", batch), ("gated face batch", gated), ("tracks", tracked), ("tracks + face batch", tracked_batch),
             ("tracks + shots", shots), ("pixelate", redacting(dict(cells=6))), ("blur", redacting(dict(blur=3))),
             ("overlay", redacting(None, "detect_overlay_device")), ("tracks + redaction", tracked_redacting("detect_redacted_device", dict(cells=6))),
             ("tracks + overlay", tracked_redacting("detect_tracked_overlay", None)))

    # the standalone calls: the first three frames that hold faces, with the faces the plain call finds in them
    found = fresh(lambda det: det.detect_device(ptrs[:7], [448] * 7, [448] * 7, 0.5))
    with_faces = [i for i in range(7) if found[i]][:3]
    assert len(with_faces) == 3
    faces = [rows_of(found[i]) for i in with_faces]
    p3, hw3 = [ptrs[i] for i in with_faces], [448] * 3

    def s_align(det, f):
        return det.align(p3, hw3, hw3, f, crop_size=112)

    def s_batch(det, f):
        return det.face_batch(p3, hw3, hw3, f, crop_size=112, dtype="f16", max_faces=8)

    def s_update(det, f):
        trk = det.tracker(3)
        try:
            return trk.update([0, 1, 2], f), trk.update([0, 1, 2], f), trk.read(1)
        finally:
            trk.close()

    def s_shots(det, f):
        trk = det.tracker(3).enable_shots(crop_size=32, dtype="u8")
        try:
            return trk.update_shots(p3, hw3, hw3, [0, 1, 2], f), trk.update_shots(p3, hw3, hw3, [2, 1, 0], f), trk.read_shots(2)
        finally:
            trk.close()

    def s_redact(det, f):
        a, b = clones(with_faces), clones(with_faces)
        red = det.redact_device([d.data_ptr() for d in a], hw3, hw3, f, spec=dict(cells=6))
        ov = det.overlay_device([d.data_ptr() for d in b], hw3, hw3, f)
        return red, ov, after(a), after(b)

    standalone = (s_align, s_batch, s_update, s_shots, s_redact)

    def refused(det, trk):
        """one refused call per stage, each in an argument check before any launch"""
        pair = [dev[0].data_ptr()] * 2
        calls = (lambda: det.detect_aligned_device(*args, 0.5, crop_size=8),
                 lambda: det.detect_face_batch_device(*args, 0.5, max_faces=4097),
                 lambda: det.detect_tracked_device(*args, trk, [N] * N, 0.5),                          # a stream out of range
                 lambda: det.detect_redacted_device(pair, [448] * 2, [448] * 2, 0.5))                  # two frames that overlap
        before = det.launch_stats()
        for call in calls:
            with pytest.raises(rfa.RFError) as e:
                call()
            assert e.value.status == -1
        # the checks of the tracker come before any state changes: it is not refused afterwards.  A frame that detect() itself refuses
        # (a row step below cols * 3) is found with the call open, and then the tracker is refused until it is reset
        first = det.detect_tracked_device(*args, trk, STREAMS, 0.5)
        for call in (lambda: det.detect_tracked_device(*args, trk, STREAMS, 0.5, steps=[1] * N), lambda: det.detect_tracked_device(*args, trk, STREAMS, 0.5),
                     lambda: trk.read(0)):
            with pytest.raises(rfa.RFError) as e:
                call()
            assert e.value.status == -1
        assert det.launch_stats()["images"] - before["images"] == N
        trk.reset(-1)
        assert frozen(det.detect_tracked_device(*args, trk, STREAMS, 0.5)) == frozen(first)

    # the references: each call on a fresh handle of its own
    first = {name: fresh(call) for name, call in steps}
    want = [frozen(first[name]) for name, _ in steps]
    alone = [fresh(call, faces) for call in standalone]
    want_alone = [frozen(r) for r in alone]
    for k in range(len(want)):                     # different results: a stale cursor, table or block would show
        assert all(want[k] != want[j] for j in range(k)), steps[k][0]
    assert all(want_alone[k] != want_alone[j] for k in range(5) for j in range(k))
    # ... and none of them is empty: faces, crops, quality records, live ids, stored shots, regions and changed pixels
    def live(tags):
        return sum(int((t["id"] > 0).sum()) for t in tags)

    def changed(frames, which=range(N)):
        return any(not np.array_equal(a, seven[i % 7]) for i, a in zip(which, frames))

    dets, crops, _ = first["align"]
    assert sum(len(d) for d in dets) == sum(len(c) for c in crops) > 0
    assert 0 < len(first["gated face batch"][1]) < len(first["face batch"][1])
    for name in ("pixelate", "blur", "overlay"):
        assert int(first[name][1].sum()) > 0 and changed(first[name][2]), name
    tags_of = {"tracks": lambda c: c[1], "tracks + face batch": lambda c: c[5], "tracks + shots": lambda c: c[0][1],
               "tracks + redaction": lambda c: c[0][1], "tracks + overlay": lambda c: c[0][1]}
    for name, tags in tags_of.items():
        one, two = first[name]
        assert live(tags(one)) > 0 and live(tags(two)) > 0, name
        # the second call met live tracks: every face kept the id the first call gave it, and the tags moved on
        assert [t["id"].tolist() for t in tags(two)] == [t["id"].tolist() for t in tags(one)] and frozen(tags(two)) != frozen(tags(one)), name
    for call in first["tracks"]:
        assert sum(len(d) for d in call[0]) > 0
    for call in first["tracks + face batch"]:
        assert len(call[1]) > 0 and sum(len(q) for q in call[4]) > 0
    for call in first["tracks + shots"]:
        assert sum(len(q) for q in call[0][5]) > 0 and any(ent.any() and (rec["id"] > 0).any() for ent, rec in call[1])
    for name in ("tracks + redaction", "tracks + overlay"):
        for _, pixels, region_counts, frames in first[name]:
            assert int(pixels.sum()) > 0 and int(region_counts.sum()) > 0 and changed(frames), name
    a_align, a_batch, a_update, a_shots, a_redact = alone
    assert sum(len(c) for c in a_align[0]) > 0 and sum(len(m) for m in a_align[1]) > 0
    assert len(a_batch[1]) > 0 and a_batch[3][-1] > 0
    assert live(a_update[0][0]) > 0 and [t["id"].tolist() for t in a_update[1][0]] == [t["id"].tolist() for t in a_update[0][0]]
    assert (a_update[2][0]["id"] > 0).any()
    assert live(a_shots[0][0]) > 0 and live(a_shots[1][0]) > 0 and a_shots[2][0].any() and (a_shots[2][1]["id"] > 0).any()
    for pixels, region_counts in a_redact[:2]:
        assert int(pixels.sum()) > 0 and int(region_counts.sum()) > 0
    assert changed(a_redact[2], with_faces) and changed(a_redact[3], with_faces)

    det = handle(rfa)
    plain = det.detect_device(ptrs, hw, hw, 0.5)
    for k, (name, call) in enumerate(steps):
        assert frozen(call(det)) == want[k], (k, name)
    trk = det.tracker(N)
    refused(det, trk)
    trk.close()
    assert [frozen(call(det, faces)) for call in standalone] == want_alone
    for k, (name, call) in reversed(list(enumerate(steps))):
        assert frozen(call(det)) == want[k], (k, name, "reverse")
    assert frozen(det.detect_device(ptrs, hw, hw, 0.5)) == frozen(plain)
    det.close()
