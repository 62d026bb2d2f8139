"""findPredelay and fixPredelay of the C++ mirror (the library's overloads in parallel-reverb-raytracer_amd/host/rayverb_api.cpp: a
partial per host thread, parallel_ranges with one thread below 1 << 16 elements and RVB_HOST_THREADS at or above) against the CPU
oracle's rvbo_find_predelay / rvbo_fix_predelay AND against the header's templates (include/rayverb/rayverb.h:43-68), which
tests/cpp/api_stages.cpp instantiates on a record type the library has no overload for.  Both the nested form (all channels) and the
per-channel form; fixPredelay without an argument and with half the predelay.  While nothing is resident the library makes no device
call, and mode=predelay never constructs a context: this runs without a GPU.  RVB_HOST_THREADS is read once per process, so every
thread count is a child process."""
import functools

import numpy as np
import pytest

import api_stages as S
from parallel_reverb_raytracer_amd.dtypes import ATTENUATED, aligned_zeros

THREADS = (1, 2, 3, 8, 64)
SEEDED = (S.THREAD_THRESHOLD - 1, S.THREAD_THRESHOLD, S.THREAD_THRESHOLD + 1, 200001)


def attenuated_with(times, seed):
    a = aligned_zeros(times.shape[0], ATTENUATED)
    a["time"] = times
    a["volume"] = np.random.default_rng(seed).uniform(-1.0, 1.0, (times.shape[0], 8)).astype(np.float32)
    return a


def seeded_times(n, seed):
    """35 % zero times, the others in 1 ms .. 2 s"""
    rng = np.random.default_rng(seed)
    t = rng.uniform(1e-3, 2.0, n).astype(np.float32)
    t[rng.random(n) < 0.35] = 0
    return t


@functools.lru_cache(maxsize=None)
def vectors():
    """name -> two channels of equal length.  Degenerate vectors: the second channel holds the first one's times doubled and in reverse
    order (its earliest time is another one, at the other end); seeded vectors: two seeds."""
    out = {}
    for name, t in S.degenerate_times().items():
        out[name] = [attenuated_with(t, 1), attenuated_with((t * np.float32(2))[::-1], 2)]
    for n in SEEDED:
        out["seeded_%d" % n] = [attenuated_with(seeded_times(n, n), 3), attenuated_with(seeded_times(n, n + 1), 4)]
    return out


@functools.lru_cache(maxsize=None)
def inputs(tmp, name):
    for c, a in enumerate(vectors()[name]):
        S.write("%s/%s_%d.bin" % (tmp, name, c), a)
    return "%s/%s_" % (tmp, name)


_expected = {}


def expected(oracle, name):
    """By the oracle, once per vector: find [1 + channels] (all channels, then each), and the times after fixPredelay of all channels,
    of each channel by its own predelay, and of all channels by half the predelay."""
    if name not in _expected:
        chans = vectors()[name]
        find = np.asarray([oracle.find_predelay(chans)] + [oracle.find_predelay([c]) for c in chans], np.float32)
        forms = {"nested": [find[0]] * len(chans), "each": list(find[1:]), "half": [find[0] * np.float32(0.5)] * len(chans)}
        times = {}
        for form, seconds in forms.items():
            fixed = [c.copy() for c in chans]
            for c, s in zip(fixed, seconds):
                oracle.fix_predelay(c, float(s))
            times[form] = [c["time"].copy() for c in fixed]
        _expected[name] = (find, times)
    return _expected[name]


def test_the_vectors_hold_what_they_are_built_for():
    v = vectors()
    for n in SEEDED:
        for c in v["seeded_%d" % n]:
            zero = np.count_nonzero(c["time"] == 0) / float(n)
            assert c.shape[0] == n and 0.33 < zero < 0.37
    assert v["empty"][0].shape[0] == 0 and v["one"][0].shape[0] == 1 and not v["zero_times"][0]["time"].any()
    for name in ("last_only", "big_last_only"):
        t = v[name][0]["time"]
        assert np.flatnonzero(t).tolist() == [t.shape[0] - 1]
    t = v["big_first_of_last_range"][0]["time"]
    assert t.shape[0] == 2 * S.THREAD_THRESHOLD and np.flatnonzero(t).tolist() == [t.shape[0] - t.shape[0] // 8]
    t = v["negative_zeros"][0]["time"]
    assert np.signbit(t[0]) and np.signbit(t[-1]) and (t >= 0).all() and np.count_nonzero(t > 0) > 100 and not np.isnan(t).any()


@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("name", sorted(S.degenerate_times()) + ["seeded_%d" % n for n in SEEDED])
def test_library_predelay_equals_the_oracle_and_the_header_templates(oracle, tmp_path_factory, tmp_path, name, threads):
    prefix = inputs(str(tmp_path_factory.getbasetemp()), name)
    find, times = expected(oracle, name)
    if name.startswith("seeded") or name in ("one", "last_only", "big_last_only", "big_first_of_last_range", "negative_zeros"):
        assert find[0] > 0
    else:
        assert find[0] == 0                  # empty, all times zero: fixPredelay changes nothing
        assert all(np.array_equal(t, c["time"]) for t, c in zip(times["nested"], vectors()[name]))
    out = S.run(tmp_path, {"RVB_HOST_THREADS": str(threads)}, mode="predelay", channels=2, **{"in": prefix})
    assert out.split() == ["touched", "0"], "a volume or a padding word changed: " + out
    for who in ("library", "template"):
        got = S.read(tmp_path, who + "_find.bin", np.float32)
        # == : the reference leaves the sign of a zero result to the element order
        assert got.shape == find.shape and (got == find).all(), "%s findPredelay: %r, the oracle has %r" % (who, got, find)
        for form, want in times.items():
            for c, w in enumerate(want):
                got = S.read(tmp_path, "%s_%s_%d.bin" % (who, form, c), np.float32)
                assert got.shape == w.shape and np.array_equal(got.view(np.uint32), w.view(np.uint32)), (who, form, c, S.first_difference(got, w))
