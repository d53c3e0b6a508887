"""tests/schedule_ref.py on the CPU: the closing-rule model against schedules worked out by hand (not against the engine), the pool's
layout, and the key."""
import numpy as np

import schedule_ref as sr
from retinaface_amd.detector import Detection


def test_model_fill_and_overflow_example_a():
    """cap 16, one threshold.  4+3+4+1+4 = 16: launched at once when the fifth ticket joins.  2+4+4+1+3 = 14; the last ticket of 4 would
    make 18, so the 14 go first and the 4 wait for the first rf_wait."""
    sizes = [4, 3, 4, 1, 4, 2, 4, 4, 1, 3, 4]
    got = sr.expected_launches([(n, 0.5) for n in sizes], 16)
    assert got == [16, 14, 4] and sum(got) == sum(sizes) == 34


def test_model_threshold_changes_example_b():
    """cap 16, nine tickets of 2 images: a launch per run of equal thresholds, none of them full."""
    thr = [.5, .5, .1, .1, .1, .02, .5, .5, .02]
    got = sr.expected_launches([(2, t) for t in thr], 16)
    assert got == [4, 6, 2, 4, 2] and sum(got) == 18


def test_model_exact_fill_launches_at_once_and_the_next_ticket_opens_a_new_super_batch():
    assert sr.expected_launches([(4, .5)] * 4, 16) == [16]                        # exactly cap: nothing is left pending
    assert sr.expected_launches([(4, .5)] * 4 + [(1, .5)], 16) == [16, 1]         # ... and the next ticket does not join it
    assert sr.expected_launches([(4, .5)] * 3 + [(3, .5), (1, .5), (1, .5)], 16) == [16, 1]
    assert sr.expected_launches([(4, .5)] * 3 + [(3, .5), (2, .5)], 16) == [15, 2]      # 15 + 2 > 16: closed one short of full
    assert sr.expected_launches([(1, .5), (1, .1), (1, .5)], 16) == [1, 1, 1]     # a threshold that comes back is still a change
    assert sr.expected_launches([], 16) == []
    assert sr.expected_launches([(4, .5), (4, .1)], 4) == [4, 4]                  # cap = one ticket: every ticket fills a launch


def test_pool_layout(base_frame):
    pool = sr.POOL(base_frame)
    assert [f.name for f in pool] == ["fit0", "fit1", "fit2", "fit3", "fit4", "fit5", "small0", "small1", "big0", "big1", "odd", "empty"]
    assert [sr.shape(f) for f in pool] == [sr.NET_HW] * 6 + [(70, 100)] * 2 + [(192, 256)] * 2 + [(131, 150), (0, 0)]
    assert all(sr.shape(pool[i]) == sr.NET_HW for i in sr.FIT)
    assert pool[sr.BIG[0]].img.shape[0] == 2 * sr.NET_HW[0] and pool[sr.BIG[0]].img.shape[1] == 2 * sr.NET_HW[1]
    # distinct frames: a result delivered under the wrong ticket cannot pass for the right one
    imgs = [f.img.tobytes() for f in pool if f.img is not None]
    assert len(set(imgs)) == len(imgs)
    # the strided frame: odd byte offset, a row step that is odd and larger than cols * 3, the view's pixels are the dense frame's
    s = pool[sr.SMALL_STRIDED]
    assert s.offset % 2 == 1 and s.step % 2 == 1 and s.step > 300 and s.img.strides == (s.step, 3, 1)
    assert s.img.ctypes.data == s.back.ctypes.data + s.offset
    assert np.array_equal(s.img, sr.edge_frame(base_frame, (70, 100), 1))
    assert s.offset + 69 * s.step + 300 <= s.back.size
    for f in pool:                                   # every other frame is dense and starts its buffer
        if f.img is not None and f is not s:
            assert f.offset == 0 and f.step == f.img.shape[1] * 3 and f.img.flags.c_contiguous
    e = pool[sr.EMPTY]
    assert e.img is None and sr.host_image(e).shape == (0, 0, 3)
    assert sr.edge_frame(base_frame, (64, 96), 3).shape == (64, 96, 3)


def test_key_sees_every_byte():
    d = Detection(0.9, (1.0, 2.0, 3.0, 4.0), (1.0,) * 5, (2.0,) * 5, 7)
    e = Detection(0.9, (1.0, 2.0, 3.0, np.nextafter(np.float32(4.0), np.float32(5.0))), (1.0,) * 5, (2.0,) * 5, 7)
    a = Detection(0.9, (1.0, 2.0, 3.0, 4.0), (1.0,) * 5, (2.0,) * 5, 8)
    assert sr.key([d], 3) == sr.key([d], 3)
    assert sr.key([d], 3) != sr.key([e], 3) and sr.key([d], 3) != sr.key([a], 3) and sr.key([d], 3) != sr.key([d], 4)
    assert sr.key([], 0) == ((), (), 0) and sr.key([d, a], 3) != sr.key([a, d], 3)
