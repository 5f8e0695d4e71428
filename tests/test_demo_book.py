"""CPU: the bookkeeping of the demos' loop (mladversarialobjectdetection_amd/demo.py: Demo, AttackDemo,
RecoveryDemo restated from the reference's demo.py:51-59, 98-105, 123-125, 159-165, 187-190) on
hand-written score sequences against hand-computed answers.  Scores are fractions in [0, 1], as the
detector reports them; every value used here is chosen so that its float32 product with 100 is known
exactly (k / 64 and k / 256 fractions, and the float32 neighbours of 55 / 100 found by stepping)."""
import numpy as np

from mladversarialobjectdetection_amd.demo import SCORE_THRESH, AttackDemo, Demo, RecoveryDemo

F = np.float32


def _frac(percent, direction=0):
    """A float32 score whose float32 product with 100 is exactly `percent` (direction 0), or the
    nearest product above (+1) / below (-1) it."""
    s = F(percent) / F(100.)
    while s * F(100.) > F(percent):
        s = np.nextafter(s, F(0))
    while s * F(100.) < F(percent):
        s = np.nextafter(s, F(1))
    assert s * F(100.) == F(percent)
    while direction > 0 and s * F(100.) <= F(percent):
        s = np.nextafter(s, F(1))
    while direction < 0 and s * F(100.) >= F(percent):
        s = np.nextafter(s, F(0))
    return s


def test_threshold_is_the_references_int():
    assert Demo("x").thresh == int(SCORE_THRESH * 100.) == 55
    assert Demo("x", min_score_thresh=0.5).thresh == 50


def test_mean_score_half_even_no_person_and_float64():
    d = Demo("clean")
    # 0.125 -> 12.5 -> 12 (half to even), then (0.125 + 0.625) / 2 = 0.375 -> 37.5 -> 38
    assert d.measure_mean_score([F(0.125), F(0.0625)]) == 12
    assert d.measure_mean_score([F(0.625)]) == 38
    # a frame without a person counts as 0: (0.125 + 0.625 + 0) / 3 = 25
    assert d.measure_mean_score([]) == 25
    assert isinstance(d.measure_mean_score([]), int)
    # the mean is taken in float64 (the documented deviation): 0.125 and its float32 successor
    # 0.125 + 2^-26 average to 0.125 + 2^-27, 12.5000007 % -> 13; a float32 sum would round the
    # 2^-26 away (a tie to even at 0.25) and give 12.5 -> 12
    d = Demo("clean")
    d.measure_mean_score([F(0.125)])
    assert d.measure_mean_score([np.nextafter(F(0.125), F(1))]) == 13
    # run returns the frame's own score in float32 percent
    mean_sc, sc = Demo("clean").run([F(0.25), F(0.75), F(0.5)])
    assert mean_sc == 75 and sc == F(75.) and sc.dtype == np.float32
    mean_sc, sc = Demo("clean").run([])
    assert mean_sc == 0 and sc == 0. and sc.dtype == np.float32


def test_asr_queue_and_threshold_edges():
    a = AttackDemo("adv. patch")
    assert a.calc_asr() is None  # empty queue: nothing to divide by
    at, above, below = _frac(55.), _frac(55., +1), _frac(55., -1)
    assert at * F(100.) == F(55.) and above * F(100.) > F(55.) > below * F(100.)
    # clean score exactly 55: not above the threshold, the frame is not counted
    _, sc, counted, success = a.run([F(0.25)], at * F(100.))
    assert sc == F(25.) and not counted and not success and a.calc_asr() is None
    # no person on the clean frame (score 0): not counted
    assert a.run([], F(0.))[2:] == (False, False) and a.calc_asr() is None
    # clean score just above 55: counted; attacked score exactly 55 is not a success
    _, sc, counted, success = a.run([at], above * F(100.))
    assert sc == F(55.) and counted and not success and a.calc_asr() == 0
    # attacked score just below 55: a success -> 1 of 2 = 50
    _, sc, counted, success = a.run([below, F(0.125)], F(90.))
    assert sc < F(55.) and counted and success and a.calc_asr() == 50
    # attacked frame without a person: score 0, a success -> 2 of 3 = 66.67 -> 67
    assert a.run([], F(90.))[1:] == (F(0.), True, True) and a.calc_asr() == 67
    # 1 of 8 = 12.5 -> 12 (half to even)
    b = AttackDemo("b")
    b.run([F(0.25)], F(80.))
    for _ in range(7):
        b.run([F(0.75)], F(80.))
    assert b.calc_asr() == 12
    # the mean runs over every frame, counted or not: (25 + 0 + 55 + below + 0) / 5
    assert a._sc_arr == [F(0.25), F(0.), at, below, F(0.)]
    assert len(a._atk_queue) == 3


def test_adr_queue_and_delta_edges():
    r = RecoveryDemo("recovery")
    assert r.calc_adr() is None
    # clean score at the threshold: not counted, whatever the recovery gained
    _, sc_after, counted, detected = r.run([F(0.75)], F(10.), F(55.))
    assert sc_after == F(75.) and not counted and not detected and r.calc_adr() is None
    # delta exactly 10 (62.5 - 52.5): not detected
    _, sc_after, counted, detected = r.run([F(0.625)], F(52.5), F(90.))
    assert sc_after - F(52.5) == F(10.) and counted and not detected and r.calc_adr() == 0
    # delta just above 10
    down = np.nextafter(F(52.5), F(0.))  # 52.5 - 2^-18: the float32 difference is 10 + 2^-18 exactly
    _, sc_after, counted, detected = r.run([F(0.625)], down, F(90.))
    assert sc_after - down > F(10.) and counted and detected and r.calc_adr() == 50
    # the recovered frame has no person: delta negative
    assert r.run([], F(30.), F(56.))[1:] == (F(0.), True, False) and r.calc_adr() == 33
    assert [float(x) for x in r._diff_queue[:1]] == [10.0] and len(r._diff_queue) == 3
    # a custom detection threshold
    r2 = RecoveryDemo("r", atk_detection_thresh=5.)
    assert r2.run([F(0.5)], F(44.), F(90.))[3] is True and r2.calc_adr() == 100
