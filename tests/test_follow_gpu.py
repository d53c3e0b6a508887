"""Followed tracks on the GPU: follow_keep_kernel, follow_search_kernel and follow_step_kernel against tests/follow_ref.py and against
the host entry points, byte for byte (followed faces, tags, ended lists, counts, tables, records and templates), through
Tracker.update_follow / Tracker.follow_device; the fused key call against the plain tracked call; the key / follow schedule; the
refusals; and the C++ class."""
import os
import subprocess

import numpy as np
import pytest

import follow_ref as fr
import track_ref as tr
from conftest import ASSETS, ROOT
from test_follow_host import FollowHost, boxes_for, canvas, pan_windows, strided
from test_gpu_align import FP16, engine, rfa, rows_of, to_device  # noqa: F401  (rfa: fixture)
from test_track_gpu import check_tables, tr_scale
from test_track_host import by_score, face

pytestmark = pytest.mark.gpu
f32 = np.float32
EMPTY = np.zeros(0, tr.FACE)


class DevFrame:
    """a host frame (rows of `step` bytes, odd base address) and the same bytes in device memory at the same offset"""

    def __init__(self, host):
        import torch
        self.host = host
        if host is None:
            self.ptr, self.rows, self.cols, self.step = 0, 0, 0, 0
            return
        buf = host.base                                            # strided()'s whole buffer
        self.dev = torch.from_numpy(buf.copy()).cuda()
        torch.cuda.synchronize()
        self.ptr = self.dev.data_ptr() + (host.ctypes.data - buf.ctypes.data)
        self.rows, self.cols, self.step = host.shape[0], host.shape[1], host.strides[0]


def args_of(frames):
    return [f.ptr for f in frames], [f.rows for f in frames], [f.cols for f in frames]


def steps_of(frames):
    return [f.step for f in frames]


def check_follow_state(trk, refs, hosts=None):
    check_tables(trk, refs)
    for s, ref in enumerate(refs):
        rec, tpl = trk.read_follow(s)
        assert rec.tobytes() == ref.records.tobytes(), (s, rec, ref.records)
        assert tpl.tobytes() == fr.read_templates(ref).tobytes(), s
        if hosts is not None:
            assert rec.tobytes() == hosts[s].records.tobytes() and tpl.tobytes() == hosts[s].masked_templates().tobytes(), s
            assert trk.read(s)[0].tobytes() == hosts[s].table.tobytes(), s


def key_call(trk, refs, hosts, streams, frames, per_image, cap_ended=8):
    cap = max([len(f) for f in per_image] + [1])
    tags, ended = trk.update_follow(*args_of(frames), streams, per_image, steps=steps_of(frames), cap_per_image=cap, cap_ended=cap_ended)
    for i, s in enumerate(streams):
        if s < 0:
            assert not trk.last_tags[i].view(np.uint8).any() and trk.last_ended_counts[i] == 0
            continue
        rtags, rended, _ = fr.key_step(refs[s], frames[i].host, per_image[i])
        assert tags[i].tobytes() == rtags.tobytes(), i
        assert trk.last_ended_counts[i] == len(rended) and ended[i].tobytes() == rended[:cap_ended].tobytes(), i
        if hosts is not None:
            hosts[s].key(frames[i].host, per_image[i], cap_ended=cap_ended)
    check_follow_state(trk, refs, hosts)


def follow_call(trk, refs, hosts, streams, frames, cap=None, cap_ended=8):
    faces, tags, ended = trk.follow_device(*args_of(frames), streams, steps=steps_of(frames), cap_per_image=cap, cap_ended=cap_ended)
    cap = trk.max_tracks if cap is None else cap
    cut = False
    for i, s in enumerate(streams):
        if s < 0:
            assert trk.last_counts[i] == 0 and not trk.last_tags[i].view(np.uint8).any() and trk.last_ended_counts[i] == 0
            continue
        rout, rtags, rended = fr.follow_step(refs[s], frames[i].host)
        assert trk.last_counts[i] == len(rout) and trk.last_ended_counts[i] == len(rended), i
        assert faces[i].tobytes() == rout[:cap].tobytes() and tags[i].tobytes() == rtags[:cap].tobytes(), i
        assert ended[i].tobytes() == rended[:cap_ended].tobytes(), i
        cut = cut or len(rout) > cap or len(rended) > cap_ended
        if hosts is not None:
            hosts[s].follow(frames[i].host, cap, cap_ended)
    assert trk.truncated == cut
    check_follow_state(trk, refs, hosts)
    return faces, tags, ended


def grid_faces(n, rows, cols):
    """n small boxes on a grid, far enough apart to open a track each; q = 1"""
    per_row = cols // 15
    return by_score([face(0.99 - 0.003 * j, 2.0 + 15 * (j % per_row), 1.0 + 12 * (j // per_row), 10.0) for j in range(n)])


# ---------------------------------------------------------------------------------------------- 1. constructed cases
@pytest.mark.parametrize("max_tracks,n_streams,radius", ((4, 8, 16), (64, 3, 8), (256, 1, 3)))
def test_key_and_follow_calls_equal_the_reference_and_the_host(rfa, max_tracks, n_streams, radius):
    """every slot live (4: boxes over the edges, larger than the frame, q = 1, 2 and more; 64 and 256: a grid), then free slots between
    live ones; 1, 3 and 8 streams in a call, an image of stream -1, a frame without pixels"""
    det = engine(rfa)
    rows, cols = (200, 240) if max_tracks > 4 else (96, 128)
    kw = dict(max_tracks=max_tracks, max_missed=1, min_hits=2)
    fkw = dict(radius=radius, max_mad=40, max_run=3)
    trk = det.tracker(n_streams, follow=fkw, **kw)
    refs = [fr.Stream(tr.Spec(**kw), fr.FollowSpec(**fkw)) for _ in range(n_streams)]
    hosts = [FollowHost(det._lib, max_tracks, radius, 40, 3, max_missed=1, min_hits=2) for _ in range(n_streams)]
    bigs = [canvas(rows + 60, cols + 60, 100 * max_tracks + s) for s in range(n_streams)]
    if max_tracks == 4:
        sets = [by_score([face(0.9 - 0.01 * i, *b) for i, b in enumerate(boxes_for(rows, cols)[(3 * s) % 7:][:4])]) for s in range(n_streams)]
    else:
        sets = [grid_faces(max_tracks, rows, cols) for _ in range(n_streams)]
    streams = list(range(n_streams))

    def frames_at(x0, y0, with_untracked=True):
        fs = [DevFrame(strided(bigs[s][y0:y0 + rows, x0:x0 + cols])) for s in range(n_streams)]
        return (fs + [fs[0]], streams + [-1]) if with_untracked else (fs, streams)

    try:
        x0, y0 = 30, 30
        fs, st = frames_at(x0, y0)
        key_call(trk, refs, hosts, st, fs, sets + [sets[0]])
        assert all(int((r.table["id"] != 0).sum()) == max_tracks for r in refs)                # every slot live
        for _ in range(2):
            x0, y0 = x0 + 2, y0 - 1
            fs, st = frames_at(x0, y0)
            faces, tags, _ = follow_call(trk, refs, hosts, st, fs)
        assert sum(len(f) for f in faces) > 0
        # a key step without every third face: their tracks miss once, then end on a follow step: free slots between live ones
        fs, st = frames_at(x0, y0, False)
        thinned = [by_score(tr.rows_of(f)[np.arange(len(f)) % 3 != 1]) for f in sets]
        key_call(trk, refs, hosts, st, fs, thinned)
        for k in range(3):
            x0, y0 = x0 - 3, y0 + 2
            fs, st = frames_at(x0, y0)
            if k == 1:
                fs[0] = DevFrame(None)                                                          # no pixels: every track of stream 0 ages
            follow_call(trk, refs, hosts, st, fs, cap_ended=max_tracks)
        live = refs[-1].table["id"] != 0
        assert 0 < live.sum() < max_tracks and (max_tracks == 4 or not live[1])
        # a cut output list and a cut ended list
        fs, st = frames_at(x0, y0, False)
        key_call(trk, refs, hosts, st, fs, sets)
        follow_call(trk, refs, hosts, st, fs, cap=1 if max_tracks > 4 else 0)
        # flush ends the live tracks and zeroes their records; reset: empty tables, zero records
        want = tr.flush(refs[0])
        refs[0].records[:] = np.zeros((), fr.FOLLOW)
        assert trk.flush(0).tobytes() == want.tobytes()
        check_follow_state(trk, refs)
        trk.reset(-1)
        check_follow_state(trk, [fr.Stream(tr.Spec(**kw)) for _ in range(n_streams)])
    finally:
        trk.close()


def test_host_frames_follow_like_device_frames(rfa):
    det = engine(rfa)
    trk = det.tracker(2, follow=True, max_tracks=8)
    refs = [fr.Stream(tr.Spec(max_tracks=8)) for _ in range(2)]
    big = canvas(160, 200, 77)
    try:
        a = [DevFrame(strided(big[20:116, 20:148])), DevFrame(strided(big[30:126, 40:168]))]
        faces = [by_score([face(0.9, 40, 30, 31), face(0.8, 80, 20, 20)]), by_score([face(0.9, 20.5, 10.2, 32)])]
        key_call(trk, refs, None, [0, 1], a, faces)
        b = [strided(big[29:125, 38:166]), strided(big[22:118, 23:151])]                 # stream 1's next frame, then stream 0's
        got, tags, _ = trk.follow(b + [None], [1, 0, -1])
        for i, s in ((0, 1), (1, 0)):
            rout, rtags, _ = fr.follow_step(refs[s], b[i])
            assert got[i].tobytes() == rout.tobytes() and tags[i].tobytes() == rtags.tobytes() and len(rout) > 0
        check_follow_state(trk, refs)
    finally:
        trk.close()


# ---------------------------------------------------------------------------------------------- 2. refusals
def test_refusals_leave_tracker_and_handle_usable(rfa, crop448):
    det = engine(rfa)
    dev = to_device([crop448])[0]
    args = ([dev.data_ptr()], [448], [448])
    two = ([dev.data_ptr()] * 2, [448] * 2, [448] * 2)
    one_face = [by_score([face(0.9, 100, 100, 60)])]
    trk, plain, stepped = det.tracker(2, max_tracks=4), det.tracker(1, max_tracks=4), det.tracker(1, max_tracks=4)
    shots, motion = det.tracker(1, max_tracks=4), det.tracker(1, max_tracks=4, motion=True)
    try:
        def refused(call, status=-1):
            with pytest.raises(rfa.RFError) as e:
                call()
            assert e.value.status == status

        for bad in (dict(radius=17), dict(radius=-1), dict(max_mad=256), dict(max_run=65537)):
            refused(lambda: trk.enable_follow(**bad))
        stepped.update([0], one_face)
        refused(lambda: stepped.enable_follow())                                         # it has stepped a frame
        shots.enable_shots(crop_size=16, dtype="u8")
        refused(lambda: shots.enable_follow())                                           # no composition yet, either way round
        refused(lambda: motion.enable_follow())
        trk.enable_follow(radius=4)
        refused(lambda: trk.enable_follow())                                             # twice
        refused(lambda: trk.enable_shots(crop_size=16, dtype="u8"))
        refused(lambda: trk.enable_motion())
        # every plain tracked call refuses a tracker with follow, every follow call a tracker without: nothing changes
        trk.update_follow(*args, [0], one_face)
        before = (trk.read(0)[0].tobytes(), trk.read(0)[1], trk.read_follow(0)[0].tobytes(), trk.read_follow(0)[1].tobytes())
        assert trk.read_follow(0)[0][0]["valid"] == 1
        refused(lambda: trk.update([0], one_face))
        refused(lambda: det.detect_tracked_device(*args, trk, [0], 0.5))
        refused(lambda: det.detect_tracked([crop448], trk, [0], 0.5))
        refused(lambda: det.detect_track_face_batch_device(*args, trk, [0], 0.5))
        refused(lambda: trk.detect_redacted_device(*args, [0], 0.5))
        refused(lambda: trk.detect_tracked_overlay(*args, [0], 0.5))
        refused(lambda: plain.update_follow(*args, [0], one_face))
        refused(lambda: plain.follow_device(*args, [0]))
        refused(lambda: det.detect_track_follow_device(*args, plain, [0], 0.5))
        refused(lambda: plain.read_follow(0))
        # a stream named twice, a stream out of range, a row step below cols * 3
        refused(lambda: trk.follow_device(*two, [0, 0]))
        refused(lambda: trk.update_follow(*two, [1, 1], one_face * 2))
        refused(lambda: det.detect_track_follow_device(*two, trk, [0, 0], 0.5))
        refused(lambda: trk.follow_device(*args, [2]))
        refused(lambda: trk.read_follow(2))
        refused(lambda: trk.follow_device(*args, [0], steps=[448 * 3 - 1]))
        lib, h = det._lib, det._h
        assert lib.rf_track_follow_device(h, trk._t, None, None, None, None, 1, None, None, 1, None, None, None, 0, None) == -1
        assert lib.rf_track_follow_update_device(h, trk._t, None, None, None, None, 1, None, None, 1, None, None, None, None, None, 0, None) == -1
        assert before == (trk.read(0)[0].tobytes(), trk.read(0)[1], trk.read_follow(0)[0].tobytes(), trk.read_follow(0)[1].tobytes())
        # and it still works
        faces, tags, _ = trk.follow_device(*args, [0])
        assert len(faces[0]) == 1 and tags[0][0]["flags"] & fr.FOLLOWED and trk.follow_last_launch_ms() > 0
        assert faces[0].tobytes() == before[0][56:116]                                  # the same frame: the box did not move
        # a tracker without follow still produces the plain tracker's bytes
        ref = [tr.Stream(tr.Spec(max_tracks=4))]
        tags, _ = plain.update([0], one_face)
        rtags, _, _ = tr.step(ref[0], one_face[0])
        assert tags[0].tobytes() == rtags.tobytes()
        check_tables(plain, ref)
    finally:
        for t in (trk, plain, stepped, shots, motion):
            t.close()


def test_host_memory_as_a_device_frame_is_refused_where_residency_is_looked_up(rfa, crop448):
    """as for the detection calls: a handle looks frame pointers up only when frames could live elsewhere (several devices, or
    RF_FORCE_SCATTER=1 as the one-GPU rehearsal); there a host pointer is refused before any launch and everything stays usable"""
    os.environ["RF_FORCE_SCATTER"] = "1"
    det = None
    try:
        det = rfa.RetinaFace(ASSETS, "net3", 0.4, precision=FP16, net_hw=(448, 448), model_stem="mnet25")
        trk = det.tracker(1, follow=True, max_tracks=4)
        dev = to_device([crop448])[0]
        host = np.ascontiguousarray(crop448)
        one_face = [by_score([face(0.9, 100, 100, 60)])]
        for call in (lambda: trk.follow_device([host.ctypes.data], [448], [448], [0]),
                     lambda: trk.update_follow([host.ctypes.data], [448], [448], [0], one_face)):
            with pytest.raises(rfa.RFError) as e:
                call()
            assert e.value.status == -1
        assert trk.read(0)[1] == 0
        trk.update_follow([dev.data_ptr()], [448], [448], [0], one_face)
        faces, _, _ = trk.follow_device([dev.data_ptr()], [448], [448], [0])
        assert len(faces[0]) == 1
    finally:
        os.environ.pop("RF_FORCE_SCATTER", None)
        if det is not None:
            det.close()


# ---------------------------------------------------------------------------------------------- 3. the fused key call and the schedule
def test_fused_key_call_is_the_plain_tracked_call_plus_templates(rfa, base_frame):
    det = engine(rfa)
    wins = [np.ascontiguousarray(base_frame[40 + 6 * i:488 + 6 * i, 400 + 9 * i:848 + 9 * i]) for i in range(8)]
    dev = to_device(wins)
    args = ([d.data_ptr() for d in dev], [448] * 8, [448] * 8)
    streams = [3, 0, 7, -1, 5, 1, 2, 6]
    trk, plain = det.tracker(8, follow=True), det.tracker(8)
    try:
        for call in range(2):
            want = det.detect_tracked_device(*args, plain, streams, 0.5)
            want_bufs = (plain.last_tags.tobytes(), plain.last_ended.tobytes(), plain.last_ended_counts.tobytes(), det.last_out.tobytes())
            got = det.detect_track_follow_device(*args, trk, streams, 0.5)
            assert got[0] == want[0] and sum(len(d) for d in got[0]) >= 8
            assert (trk.last_tags.tobytes(), trk.last_ended.tobytes(), trk.last_ended_counts.tobytes(), det.last_out.tobytes()) == want_bufs
            for i, s in enumerate(streams):
                if s < 0:
                    continue
                table = trk.read(s)[0]
                assert table.tobytes() == plain.read(s)[0].tobytes()
                rec, tpl = trk.read_follow(s)
                named = {int(g["slot"]) for g in got[1][i] if g["slot"] >= 0}
                assert named and set(np.nonzero(rec["valid"])[0]) == named
                for slot in named:
                    last = table[slot]["last"]
                    q, ox, oy = fr.geometry([last["x1"], last["y1"], last["x2"], last["y2"]])
                    assert (int(rec[slot]["q"]), int(rec[slot]["ox"]), int(rec[slot]["oy"]), int(rec[slot]["run"])) == (q, ox, oy, 0)
                    assert tpl[slot].tobytes() == fr.template(wins[i], q, ox, oy).tobytes(), (i, slot)
        # host frames: the same bytes
        trk.reset(-1)
        plain.reset(-1)
        want = det.detect_tracked(wins, plain, streams, 0.5)
        got = det.detect_followed(wins, trk, streams, True, 0.5)
        assert got[0] == want[0] and trk.last_tags.tobytes() == plain.last_tags.tobytes()
        assert all(trk.read_follow(s)[0]["valid"].sum() > 0 for s in streams if s >= 0)
    finally:
        trk.close()
        plain.close()


def test_key_follow_follow_follow_schedule_twice_over(rfa, base_frame):
    """the pan of the host claim test on the device: key frames through the fused call, the frames in between through follow_device,
    against the reference driven with the faces the key calls returned"""
    det = engine(rfa)
    wins = pan_windows(base_frame)
    dev = to_device(wins)
    trk = det.tracker(1, follow=True)
    ref = [fr.Stream(tr.Spec())]
    try:
        for t, w in enumerate(wins):
            a = ([dev[t].data_ptr()], [448], [448])
            if t % 4 == 0:
                got, tags, _ = det.detect_track_follow_device(*a, trk, [0], 0.5)
                assert len(got[0]) == 2
                rtags, _, _ = fr.key_step(ref[0], w, tr.faces_array(rows_of(got[0])), tr_scale(det, 448, 448))
                assert tags[0].tobytes() == rtags.tobytes()
            else:
                faces, tags, _ = trk.follow_device(*a, [0])
                rout, rtags, _ = fr.follow_step(ref[0], w)
                assert len(rout) == 2 and faces[0].tobytes() == rout.tobytes() and tags[0].tobytes() == rtags.tobytes()
            check_follow_state(trk, ref)
        assert ref[0].frames == 8 and ref[0].next_id == 3                               # two ids over the whole schedule
    finally:
        trk.close()


# ---------------------------------------------------------------------------------------------- 4. the C++ class
def test_cpp_class_follow_schedule(rfa, base_frame, tmp_path):
    src = os.path.join(ROOT, "tests", "csrc", "test_follow.cpp")
    exe = str(tmp_path / "test_follow")
    lib_dir = os.path.dirname(rfa.lib_path())
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-DRF_NO_OPENCV", "-I" + os.path.join(ROOT, "include"), "-o", exe, src,
                           "-L" + lib_dir, "-lretinaface_amd", "-Wl,-rpath," + lib_dir])
    wins = pan_windows(base_frame)
    raw, out = str(tmp_path / "frames.raw"), str(tmp_path / "out.bin")
    np.stack(wins).tofile(raw)
    r = subprocess.run([exe, ASSETS, "mnet25", "448", "448", raw, str(len(wins)), "0.5", out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    blob = open(out, "rb").read()
    det = engine(rfa)
    trk = det.tracker(1, follow=True)
    try:
        want = b""
        for t, w in enumerate(wins):                     # the program: a key step every fourth frame, follow steps in between, host frames
            if t % 4 == 0:
                got, _, _ = det.detect_followed([w], trk, [0], True, 0.5)
                want += np.int32(len(got[0])).tobytes() + rows_of(got[0]).tobytes()
            else:
                faces, _, _ = det.detect_followed([w], trk, [0], False)
                want += np.int32(len(faces[0])).tobytes() + faces[0].tobytes()
        assert len(want) == 8 * (4 + 2 * 60) and blob == want
    finally:
        trk.close()
