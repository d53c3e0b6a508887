"""What tests/test_schedule_gpu.py holds the coalescing scheduler (engine.cpp submit / launch_pending / wait_impl / harvest) to, numpy only:
the pool of frames every scenario draws from, the key two results are compared by, and a pure model of when a super-batch is closed
("Enqueue and wait: when a launch is closed").  tests/test_schedule_host.py pins the model on hand-worked schedules."""
from collections import namedtuple

import numpy as np

NET_HW = (96, 128)                      # the net every scheduler test runs at: small, yet three FPN levels and several tiles per kernel
T = (0.5, 0.1, 0.02)                    # the thresholds of the pool

# One pool frame.  img: the uint8 rows x cols x 3 view a host call is handed (None: the empty frame); back / offset / step: the flat
# buffer the view lives in, the byte offset of its first pixel and its row step -- what a device call uploads and points into.
PoolFrame = namedtuple("PoolFrame", "name img back offset step")


def edge_frame(base_frame, hw, k=0):
    """A frame of hw cut from the fixture photo (the photo with its mirror image below it, for heights over 896), centred on face 0 and
    shifted by k for a batch of distinct frames."""
    tall = np.concatenate([base_frame, base_frame[::-1]], axis=0)
    y0 = int(np.clip(342 - hw[0] // 2 + 5 * k, 0, tall.shape[0] - hw[0]))
    x0 = int(np.clip(517 - hw[1] // 2 + 11 * k, 0, tall.shape[1] - hw[1]))
    return np.ascontiguousarray(tall[y0:y0 + hw[0], x0:x0 + hw[1]])


def _dense(name, img):
    img = np.ascontiguousarray(img)
    return PoolFrame(name, img, img.reshape(-1), 0, img.shape[1] * 3)


def _strided(name, img, step, offset):
    """The same pixels as a view with a row step of `step` bytes that starts `offset` bytes into its buffer (0xA5 between the rows)."""
    rows, cols = img.shape[:2]
    assert step > cols * 3
    back = np.full(offset + rows * step + 64, 0xA5, np.uint8)
    view = np.ndarray((rows, cols, 3), np.uint8, back, offset, (step, 3, 1))
    view[...] = img
    return PoolFrame(name, view, back, offset, step)


def POOL(base_frame):
    """The frames of every scenario, in a fixed order: six net-sized frames, two of 70 x 100 (smaller than the net; the second a view with
    an odd row step at an odd byte offset), two of 192 x 256 (exactly 2x oversize), one of 131 x 150 (oversize by a non-integer factor) and
    the empty frame."""
    pool = [_dense(f"fit{k}", edge_frame(base_frame, NET_HW, k)) for k in range(6)]
    pool.append(_dense("small0", edge_frame(base_frame, (70, 100), 0)))
    pool.append(_strided("small1", edge_frame(base_frame, (70, 100), 1), 100 * 3 + 7, 13))
    pool += [_dense(f"big{k}", edge_frame(base_frame, (192, 256), k)) for k in range(2)]
    pool.append(_dense("odd", edge_frame(base_frame, (131, 150), 0)))
    pool.append(PoolFrame("empty", None, None, 0, 0))
    return pool


FIT = tuple(range(6))                   # indices into POOL(): the frames that fit the net exactly ...
SMALL, SMALL_STRIDED, BIG, ODD, EMPTY = 6, 7, (8, 9), 10, 11


def host_image(f):
    """What a host call is handed for a pool frame (the empty frame: a 0 x 0 array)."""
    return f.img if f.img is not None else np.zeros((0, 0, 3), np.uint8)


def shape(f):
    return (0, 0) if f.img is None else f.img.shape[:2]


def key(dets, ncand):
    """What two results of one (frame, threshold) must agree in, byte for byte: the anchor indices, every detection row, the candidate count."""
    return (tuple(int(d.anchor_index) for d in dets), tuple(d.as_row().tobytes() for d in dets), int(ncand))


def expected_launches(tickets, cap):
    """Images per launch, in launch order, of a schedule of enqueues with frames in place on the device (no staging bytes) in which every
    enqueue comes before every wait.  tickets: (images, threshold) per enqueue; cap: max_batch x coalesce.  The rules: a pending
    super-batch is launched before a ticket that would take it past cap or whose threshold differs; it is launched at once when it holds
    exactly cap images; the first wait launches what is pending."""
    launches, pending, thr = [], 0, None
    for n, t in tickets:
        assert 1 <= n <= cap
        if pending and (pending + n > cap or t != thr):
            launches.append(pending)
            pending = 0
        if not pending:
            thr = t
        pending += n
        if pending == cap:
            launches.append(pending)
            pending = 0
    if pending:
        launches.append(pending)
    return launches
