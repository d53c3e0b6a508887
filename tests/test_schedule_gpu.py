"""The coalescing scheduler (engine.cpp: submit, launch_pending, wait_impl, harvest, pick_lane, alloc_ticket, ensure_stage) against
one-frame-at-a-time detection (`-m gpu`).

The engine under test runs a 96 x 128 net with max_batch 4, coalesce 4 and 3 lanes: 16 images per launch, 12 slots, a pool of 56
tickets.  The REFERENCE is a second engine of the same model, precision and oversize_resize mode with max_batch 1, one lane, no
coalescing and no graphs, called synchronously on one device frame at a time: the simplest path through the same kernels.  Whatever a
schedule does -- tickets of several thresholds, oversize frames joining a launch of frames that fit, staging blocks that fill up or grow,
lanes collected and reused with nobody waiting, waits out of order, synchronous calls in between, graph replays -- every image's result
must equal the reference's for that (frame, threshold) byte for byte: anchor indices, detection rows and candidate count
(schedule_ref.key).  Nothing here depends on rounding: the same kernels see the same pixels.  An fp32 reference with bilinear resize is
itself held to the CPU oracle, which anchors the chain.  Launch and image counts come from rf_launch_stats and are held to the closing
rules of INTEGRATION.md (schedule_ref.expected_launches, pinned by hand-worked cases in tests/test_schedule_host.py)."""
import contextlib
import random

import numpy as np
import pytest

import schedule_ref as sr
from conftest import ASSETS
from test_gpu_parity import FP16, FP32, INT8, compare, rfa  # noqa: F401  (rfa: fixture)

pytestmark = pytest.mark.gpu

MAX_BATCH, COALESCE, LANES = 4, 4, 3
CAP = MAX_BATCH * COALESCE                      # images per launch
SLOTS = LANES * COALESCE                        # rf_num_slots()
TICKET_POOL = 4 * LANES * COALESCE + 8          # what the header says the ticket pool holds
NET_BYTES = sr.NET_HW[0] * sr.NET_HW[1] * 3     # 36864: a lane's staging block is CAP of these
PNAME = {FP32: "fp32", FP16: "fp16", INT8: "int8"}

CONFIGS = [("mnet25", FP16), ("mnet25", INT8), ("mnet-deconv-0517", FP16)]
CONFIGS_AD = CONFIGS + [("mnet25", FP32)]       # scenarios a to d also run on fp32
IDS = lambda c: f"{c[0]}-{PNAME[c[1]]}"         # noqa: E731


def new_engine(rfa, stem, prec, mode, **kw):
    opts = dict(max_batch=MAX_BATCH, coalesce=COALESCE, lanes=LANES)
    opts.update(kw)
    return rfa.RetinaFace(ASSETS, "net3", 0.4, precision=prec, net_hw=sr.NET_HW, model_stem=stem, oversize_resize=mode, **opts)


class Rig:
    """The pool on the device, the engine under test, the reference engine and the reference's key for every (frame, threshold)."""

    def __init__(self, rfa, base_frame, stem, prec, mode):
        import torch
        self.rfa, self.stem, self.prec, self.mode = rfa, stem, prec, mode
        self.pool = sr.POOL(base_frame)
        self.dev = [torch.from_numpy(f.back).cuda() if f.back is not None else None for f in self.pool]
        torch.cuda.synchronize()
        self.ref = new_engine(rfa, stem, prec, mode, max_batch=1, lanes=1, coalesce=1, use_graph=False)
        self.det = new_engine(rfa, stem, prec, mode)
        assert self.det.num_slots() == SLOTS
        self.want, self.ref_dets = {}, {}
        for i in range(len(self.pool)):
            for thr in sr.T:
                self.reference(i, thr)
        # the pool must exercise the result path: at least 3/4 of the (non-empty frame, threshold) pairs hold a detection
        pairs = [(i, thr) for i, f in enumerate(self.pool) if f.img is not None for thr in sr.T]
        hit = sum(len(self.ref_dets[p]) > 0 for p in pairs)
        print(f"schedule pool {stem} {PNAME[prec]} {mode}: the reference finds a face in {hit} of {len(pairs)} (frame, threshold) pairs")
        assert 4 * hit >= 3 * len(pairs), (stem, PNAME[prec], hit, len(pairs))
        for thr in sr.T:
            assert self.want[(sr.EMPTY, thr)] == sr.key([], 0)

    def close(self):
        self.det.close()
        self.ref.close()

    # ---- frames
    def dev_args(self, idxs):
        """(ptrs, rows, cols, steps) of pool frames in place on the device; the empty frame is a NULL pointer."""
        ptrs = [self.dev[i].data_ptr() + self.pool[i].offset if self.dev[i] is not None else 0 for i in idxs]
        rows, cols = [sr.shape(self.pool[i])[0] for i in idxs], [sr.shape(self.pool[i])[1] for i in idxs]
        return ptrs, rows, cols, [self.pool[i].step for i in idxs]

    def host_imgs(self, idxs):
        return [sr.host_image(self.pool[i]) for i in idxs]

    def reference(self, i, thr):
        """The one-frame reference call for pool frame i, remembered."""
        if (i, thr) not in self.want:
            p, r, c, s = self.dev_args([i])
            dets = self.ref.detect_device(p, r, c, thr, steps=s)[0]
            self.ref_dets[(i, thr)] = dets
            self.want[(i, thr)] = sr.key(dets, self.ref.last_candidate_counts(1)[0])
        return self.want[(i, thr)]

    # ---- calls on the engine under test
    def enqueue(self, idxs, thr, host=False):
        if host:
            t = self.det.enqueue_host(self.host_imgs(idxs), thr)
        else:
            p, r, c, s = self.dev_args(idxs)
            t = self.det.enqueue_device(p, r, c, thr, steps=s)
        return (t, tuple(idxs), thr)

    def check(self, res, idxs, thr, what):
        ncand = self.det.last_candidate_counts(len(idxs))
        assert len(res) == len(idxs) == len(ncand), what
        for j, i in enumerate(idxs):
            if self.pool[i].img is None:
                assert res[j] == [] and ncand[j] == 0, (what, j)
            assert sr.key(res[j], ncand[j]) == self.reference(i, thr), \
                (what, j, self.pool[i].name, thr, [d.anchor_index for d in res[j]], ncand[j], self.want[(i, thr)][0], self.want[(i, thr)][2])

    def wait(self, rec, what="wait"):
        t, idxs, thr = rec
        res = self.det.wait(t, len(idxs))
        self.check(res, idxs, thr, (what, t))           # last_candidate_counts after this wait must be this ticket's
        assert not self.det.truncated, (what, t)

    def sync(self, idxs, thr, host=False, what="sync"):
        if host:
            res = self.det.detectBatchImages(self.host_imgs(idxs), thr)
        else:
            p, r, c, s = self.dev_args(idxs)
            res = self.det.detect_device(p, r, c, thr, steps=s)
        self.check(res, idxs, thr, what)

    def stats(self):
        s = self.det.launch_stats()
        return s["launches"], s["images"]

    def delta(self, s0):
        s = self.stats()
        return s[0] - s0[0], s[1] - s0[1]


_rigs = {}


@contextlib.contextmanager
def shared_rig(rfa, base_frame, stem, prec, mode="area"):
    """The rig of (stem, precision, resize mode), built once.  A test that fails may leave tickets outstanding: its rig is dropped."""
    k = (stem, prec, mode)
    if k not in _rigs:
        _rigs[k] = Rig(rfa, base_frame, stem, prec, mode)
    try:
        yield _rigs[k]
    except BaseException:
        _rigs.pop(k).close()
        raise


@contextlib.contextmanager
def fresh_rig(rfa, base_frame, stem, prec, mode="area", **kw):
    """The shared rig's pool and reference with a new engine under test (lanes not built, nothing staged yet)."""
    with shared_rig(rfa, base_frame, stem, prec, mode) as rig:
        keep = rig.det
        rig.det = new_engine(rfa, stem, prec, mode, **kw)
        try:
            yield rig
        finally:
            rig.det.close()
            rig.det = keep


# --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stem", ["mnet25", "mnet-deconv-0517"])
def test_the_reference_engine_is_held_to_the_cpu_oracle(rfa, oracles, base_frame, stem):
    """fp32, oversize_resize="bilinear" (the mode the oracle restates bit for bit): the one-frame reference engine's result for every pool
    frame and threshold against the CPU oracle -- compare()'s fp32 bars, identical candidate count.  Every other test compares with
    the reference engine, so this ties the chain to the high-precision oracle."""
    with shared_rig(rfa, base_frame, stem, FP32, "bilinear") as rig:
        for i, f in enumerate(rig.pool):
            if f.img is None:
                continue
            for thr in sr.T:
                ref = oracles[stem].detect(np.ascontiguousarray(f.img), thr, 0.4, net_hw=sr.NET_HW)
                compare(rig.ref_dets[(i, thr)], ref.rows(), ref.anchor_indices(), FP32)
                assert rig.want[(i, thr)][2] == len(ref.candidates), (f.name, thr, rig.want[(i, thr)][2], len(ref.candidates))


@pytest.mark.parametrize("cfg", CONFIGS_AD, ids=IDS)
def test_a_fill_and_overflow(rfa, base_frame, cfg):
    """Example A of tests/test_schedule_host.py with device frames at one threshold: the fifth ticket fills the first launch exactly (16,
    launched at once), the eleventh would overflow the second (14 launched, 4 left pending for the first wait).  FIFO waits."""
    sizes = [4, 3, 4, 1, 4, 2, 4, 4, 1, 3, 4]
    want = sr.expected_launches([(n, 0.5) for n in sizes], CAP)
    assert want == [16, 14, 4]
    with shared_rig(rfa, base_frame, *cfg) as rig:
        s0 = rig.stats()
        recs = [rig.enqueue([(3 * j + i) % 6 for i in range(n)], 0.5) for j, n in enumerate(sizes)]
        assert rig.delta(s0) == (2, 30)                       # the last 4 images are pending: nothing has waited yet
        for r in recs:
            rig.wait(r, "a")
        assert rig.delta(s0) == (len(want), sum(want)) == (3, 34)


@pytest.mark.parametrize("cfg", CONFIGS_AD, ids=IDS)
def test_b_threshold_changes_and_lane_reuse(rfa, base_frame, cfg):
    """Example B: nine tickets of two images, no wait in between.  Each threshold change closes a launch (one RunParams serves a launch):
    5 launches on 3 lanes, so two lanes are collected into their tickets and reused before anyone waits.  Waits in reverse order, after
    every lane has run something else; the candidate counts after each wait are that ticket's."""
    thrs = [.5, .5, .1, .1, .1, .02, .5, .5, .02]
    want = sr.expected_launches([(2, t) for t in thrs], CAP)
    assert want == [4, 6, 2, 4, 2]
    with shared_rig(rfa, base_frame, *cfg) as rig:
        s0 = rig.stats()
        recs = [rig.enqueue([j % 8, (j + 3) % 8], t) for j, t in enumerate(thrs)]      # fitting and smaller frames, one of them strided
        assert rig.delta(s0) == (4, 16)
        for r in reversed(recs):
            rig.wait(r, "b")
        assert rig.delta(s0) == (len(want), sum(want)) == (5, 18)


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
@pytest.mark.parametrize("mode", ["area", "bilinear"])
@pytest.mark.parametrize("cfg", CONFIGS_AD, ids=IDS)
def test_c_an_oversize_frame_flips_the_whole_launch_to_the_canvas(rfa, base_frame, cfg, mode, host):
    """One threshold.  Ticket 1: three frames that fit.  Ticket 2: a frame that fits, a 2x oversize frame, a smaller strided frame, the
    empty frame.  Ticket 3: a frame oversize by a non-integer factor, a frame that fits.  One launch of 9 images that gains the resize
    kernel when ticket 2 joins; the oversize frames are read from the canvas, every other frame -- ticket 1's too -- must come out as in
    a launch without a resize.  (The first version of this test caught the engine reading EVERY image of such a launch from the canvas:
    a 70 x 100 frame then went through the stem's raw-row path instead of the general one, and its fp16 score differed in the 5th digit
    from the same frame detected alone.)  Then three super-batches of frames that fit (one lands on the lane whose canvas was just
    written): need_resize must not stick."""
    tickets = [[0, 1, 2], [3, sr.BIG[0], sr.SMALL_STRIDED, sr.EMPTY], [sr.ODD, 4]]
    with shared_rig(rfa, base_frame, cfg[0], cfg[1], mode) as rig:
        for thr in (0.5, 0.02):
            s0 = rig.stats()
            recs = [rig.enqueue(t, thr, host) for t in tickets]
            assert rig.delta(s0) == (0, 0)
            for k in (1, 2, 0):
                rig.wait(recs[k], "c flip")
            assert rig.delta(s0) == (1, 9)
            for rnd in range(LANES):
                recs = [rig.enqueue([5, sr.SMALL, rnd], thr, host), rig.enqueue([1, sr.SMALL_STRIDED], thr, host)]
                for r in reversed(recs):
                    rig.wait(r, "c after")
            assert rig.delta(s0) == (1 + LANES, 9 + 5 * LANES)


@pytest.mark.parametrize("cfg", CONFIGS_AD, ids=IDS)
def test_d_staging_fills_grows_and_mixes_with_frames_in_place(rfa, base_frame, cfg):
    """A new engine and host frames.
    Mixed sources first, while no lane has staged anything: a device ticket in place opens a launch on a lane without a staging
    block; the first host ticket cannot join it (launch 1: 1 image) and opens the next lane, where a second host ticket with an oversize
    frame, a ticket from a range pinned with rf_host_register and a device ticket in place join it (launch 2: 8 images, with a resize).
    Staging bytes: one net-sized frame, then five tickets of one 192 x 256 frame.  A lane's staging block holds 16 net-sized frames = 4
    of the large ones: with the first frame in it the fourth large frame does not fit, so there are 2 launches (4 and 2 images) where
    the image rule alone gives one.
    Growth: one ticket of four 300 x 400 frames, more than a whole block, while two other lanes are in flight; the block grows to that
    ticket's size, so the next ticket with staging bytes closes the launch although it has the same threshold and room for images.
    Twice: the second time the lanes have rotated and a block that was used before is replaced."""
    import torch
    with fresh_rig(rfa, base_frame, *cfg) as rig:
        det = rig.det
        # --- mixed sources
        s0 = rig.stats()
        ring = np.stack([rig.pool[i].img for i in (2, 3)]).copy()
        det.host_register(ring)
        try:
            recs = [rig.enqueue([0], 0.1), rig.enqueue([1, sr.SMALL_STRIDED], 0.1, host=True),
                    rig.enqueue([sr.BIG[1], sr.EMPTY, 4], 0.1, host=True)]
            recs.append((det.enqueue_host([ring[0], ring[1]], 0.1), (2, 3), 0.1))
            recs.append(rig.enqueue([5], 0.1))
            assert rig.delta(s0) == (1, 1)
            for k in (3, 0, 4, 2, 1):
                rig.wait(recs[k], "d mixed")
            assert rig.delta(s0) == (2, 9)
        finally:
            det.host_unregister(ring)
        # --- staging bytes close a launch
        big = 192 * 256 * 3
        assert NET_BYTES + 3 * big <= CAP * NET_BYTES < NET_BYTES + 4 * big
        s0 = rig.stats()
        recs = [rig.enqueue([0], 0.5, host=True)] + [rig.enqueue([sr.BIG[k % 2]], 0.5, host=True) for k in range(5)]
        assert sr.expected_launches([(1, 0.5)] * 6, CAP) == [6]            # the image rule alone: one launch
        assert rig.delta(s0) == (1, 4)
        for r in recs:
            rig.wait(r, "d staging")
        assert rig.delta(s0) == (2, 6)
        # --- a ticket larger than the block: the next lane's staging grows while the other two lanes are in flight
        large = [sr.edge_frame(base_frame, (300, 400), k) for k in range(4)]
        assert sum(f.nbytes for f in large) > CAP * NET_BYTES
        dl = [torch.from_numpy(f).cuda() for f in large]
        torch.cuda.synchronize()
        want = []
        for d in dl:
            dets = rig.ref.detect_device([d.data_ptr()], [300], [400], 0.5)[0]
            want.append(sr.key(dets, rig.ref.last_candidate_counts(1)[0]))
        assert sum(len(w[0]) > 0 for w in want) >= 3
        for rnd in range(2):            # the block that grows is a lane's first, then (the lanes rotate) the 16-frame block of a lane used before
            s0 = rig.stats()
            recs = [rig.enqueue([0, 1, 2, 3], 0.5, host=True), rig.enqueue([4, sr.SMALL], 0.1, host=True)]      # closed by the threshold: in flight
            t = det.enqueue_host(large, 0.5)                                   # closes the second, grows the next lane's block to its own size
            after = rig.enqueue([5, sr.BIG[0]], 0.5, host=True)                # same threshold, 6 images: only the staging rule closes the launch
            assert rig.delta(s0) == (3, 10), rnd
            res = det.wait(t, 4)
            ncand = det.last_candidate_counts(4)
            assert [sr.key(r, c) for r, c in zip(res, ncand)] == want, rnd
            for r in (after, recs[1], recs[0]):
                rig.wait(r, ("d growth", rnd))
            assert rig.delta(s0) == (4, 12), rnd
        # the grown lane is used again by ordinary tickets
        for rnd in range(LANES):
            rig.wait(rig.enqueue([rnd, sr.ODD], 0.02, host=True), "d after growth")


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_e_seeded_schedules(rfa, base_frame, cfg, seed):
    """About 200 operations per seed -- enqueues of 1 to 4 pool frames from the device or the host at one of three thresholds, waits of
    the oldest, the newest or a random outstanding ticket, synchronous calls of one frame and of 9 frames (more than max_batch: the chunks
    join super-batches) -- then a drain in random order.  Each seed runs twice on the same engine, so the second pass replays the graphs
    the first captured for every batch size the schedule produced.  Every result equals the reference; every submitted image was
    launched exactly once."""
    with shared_rig(rfa, base_frame, *cfg) as rig:
        npool = len(rig.pool)
        for rep in range(2):
            rng = random.Random(1000 * seed + 7)
            s0 = rig.stats()
            out, images = [], 0
            for op in range(200):
                what = ("e", seed, rep, op)
                u = rng.random()
                if len(out) >= SLOTS or (out and u < 0.30):
                    k = rng.choice([0, len(out) - 1, rng.randrange(len(out))])
                    rig.wait(out.pop(k), what)
                elif u < 0.88:
                    idxs = [rng.randrange(npool) for _ in range(rng.randint(1, MAX_BATCH))]
                    out.append(rig.enqueue(idxs, rng.choice(sr.T), host=rng.random() < 0.5))
                    images += len(idxs)
                elif u < 0.95:
                    rig.sync([rng.randrange(npool)], rng.choice(sr.T), host=rng.random() < 0.5, what=what)
                    images += 1
                else:
                    rig.sync([rng.randrange(npool) for _ in range(9)], rng.choice(sr.T), host=rng.random() < 0.5, what=what)
                    images += 9
                assert len(out) <= rig.det.num_slots()
            rng.shuffle(out)
            for r in out:
                rig.wait(r, ("e drain", seed, rep))
            launches, launched = rig.delta(s0)
            print(f"schedule {IDS(cfg)} seed {seed} pass {rep}: {images} images in {launches} launches")
            assert launched == images, (seed, rep)


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_f_ticket_pool_and_refusals(rfa, base_frame, cfg):
    """One-image tickets until one is refused: the refusal is an argument error that names the cause, comes after the whole ticket pool
    (4 x lanes x coalesce + 8, at least rf_num_slots()) and changes nothing -- every outstanding ticket, most of them collected from lanes
    that were reused meanwhile, delivers its exact result.  A ticket is waited for once.  A bad frame is refused while a super-batch is
    pending and leaves the pending tickets alone."""
    err = rfa._lib.RFError
    with shared_rig(rfa, base_frame, *cfg) as rig:
        det = rig.det
        s0 = rig.stats()
        recs = []
        with pytest.raises(err) as e:
            for j in range(TICKET_POOL + 4):
                recs.append(rig.enqueue([j % 11], sr.T[(j // 5) % 3]))
        assert e.value.status == rfa._lib.RF_ERR_INVALID_ARG and "too many outstanding tickets" in str(e.value)
        assert len(recs) >= det.num_slots() and len(recs) == TICKET_POOL
        with pytest.raises(err):                                   # still full
            rig.enqueue([0], 0.5)
        order = list(range(len(recs)))
        random.Random(5).shuffle(order)
        for k in order:
            rig.wait(recs[k], "f")
        assert rig.delta(s0)[1] == len(recs)
        # a second rf_wait on a ticket that has been waited for
        with pytest.raises(err) as e:
            det.wait(recs[0][0], 1)
        assert e.value.status == rfa._lib.RF_ERR_INVALID_ARG
        # step < cols * 3 while a super-batch is pending
        s0 = rig.stats()
        pend = [rig.enqueue([0, sr.SMALL], 0.1), rig.enqueue([3], 0.1)]
        p, r, c, s = rig.dev_args([1])
        with pytest.raises(err) as e:
            det.enqueue_device(p, r, c, 0.1, steps=[c[0] * 3 - 1])
        assert e.value.status == rfa._lib.RF_ERR_INVALID_ARG
        with pytest.raises(err):                                   # more than max_batch images in one ticket
            det.enqueue_device(p * 5, r * 5, c * 5, 0.1, steps=s * 5)
        assert rig.delta(s0) == (0, 0)
        last = rig.enqueue([1], 0.1)                               # the pending super-batch is still open: this joins it
        for rec in (last, pend[1], pend[0]):
            rig.wait(rec, "f pending")
        assert rig.delta(s0) == (1, 4)


@pytest.mark.parametrize("prec", [FP16, INT8], ids=["fp16", "int8"])
def test_g_truncation_is_per_ticket(rfa, base_frame, prec):
    """An engine with the smallest candidate buffer it accepts (64; smaller sizes and sizes that are no power of two are refused at
    create).  Ticket 1: frame 0 at threshold 0.001 (the CPU oracle counts 156 candidates: an overflow), ticket 2: frame 5 at 0.5 (9
    candidates).  Two launches, waited for in reverse order: the overflow is reported for ticket 1 and only for it, and each wait
    reports its own candidate counts (the true number found, the reference engine's).  Which candidates survive an overflow is not
    defined, so the detections of ticket 1 are not compared."""
    low = 0.001
    with pytest.raises(rfa._lib.RFError):
        new_engine(rfa, "mnet25", prec, "area", max_candidates=24)
    with fresh_rig(rfa, base_frame, "mnet25", prec, max_candidates=64) as rig:
        det = rig.det
        many, few = rig.reference(0, low)[2], rig.reference(5, 0.5)[2]
        assert many > 64 and 0 < few <= 24, (many, few)
        s0 = rig.stats()
        t1 = rig.enqueue([0], low)
        t2 = rig.enqueue([5], 0.5)
        assert rig.delta(s0) == (1, 1)
        rig.wait(t2, "g second")                                   # exact result, not truncated
        assert det.last_candidate_counts(1) == [few]
        det.wait(t1[0], 1)
        assert det.truncated and det.last_candidate_counts(1) == [many]
        assert rig.delta(s0) == (2, 2)
        rig.wait(rig.enqueue([5, 0], 0.5), "g after")              # the flag does not stick
