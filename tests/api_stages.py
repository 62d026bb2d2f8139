"""Helpers around tests/cpp/api_stages.cpp, the stage dumper over the C++ mirror (include/rayverb/rayverb.h): building it, writing its
inputs, running it as a child process, reading what it wrote, and the oracle's answer for every stage behind the tracer.  Also the
builders of the degenerate vectors that tests/test_gpu_cpp_stages.py and tests/test_predelay_host.py share.  A plain module: no
fixtures, nothing of it needs a GPU but running the tool in its trace and records modes."""
import os
import subprocess

import numpy as np

from parallel_reverb_raytracer_amd.dtypes import ATTENUATED, IMPULSE, SPEAKER, aligned_zeros

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "parallel-reverb-raytracer_amd")
TOOL = os.path.join(ROOT, "tests", "cpp", "_build", "api_stages")
THREAD_THRESHOLD = 1 << 16                  # parallel_ranges (host/rayverb_api.cpp): one thread below, RVB_HOST_THREADS at or above

_built = []


def build():
    """The library if it is missing (as tests/host_lib.py), then the tool with plain g++, the way tests/test_cpp_api.py builds its binary,
    unless the one that is there is newer than its source, the headers and the library; once per process."""
    if not _built:
        libraries = [os.path.join(PKG, "librayverb.so"), os.path.join(PKG, "librvb_hip.so")]
        if not all(os.path.exists(p) for p in libraries):
            subprocess.check_call(["make", "-C", PKG, "-j4"], stdout=subprocess.DEVNULL)
        source = os.path.join(ROOT, "tests", "cpp", "api_stages.cpp")
        headers = [os.path.join(ROOT, "include", "rayverb", h) for h in sorted(os.listdir(os.path.join(ROOT, "include", "rayverb")))]
        if not os.path.exists(TOOL) or os.path.getmtime(TOOL) < max(os.path.getmtime(p) for p in [source] + headers + libraries):
            os.makedirs(os.path.dirname(TOOL), exist_ok=True)
            subprocess.check_call([
                "g++", "-std=c++11", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "include", "shims"),
                source, "-o", TOOL, "-L" + PKG, "-lrayverb", "-lrvb_hip", "-Wl,-rpath," + PKG])
        _built.append(TOOL)
    return TOOL


def run(outdir, env=None, **arguments):
    """One child process; `arguments` become name=value words.  Returns its standard output."""
    os.makedirs(outdir, exist_ok=True)
    words = [build(), "out=" + str(outdir)] + ["%s=%s" % (k, v) for k, v in sorted(arguments.items())]
    full = dict(os.environ)
    for k in ("RVB_API_RESIDENT", "RVB_HOST_THREADS", "RVB_DEVICES"):
        full.pop(k, None)
    full.update(env or {})
    done = subprocess.run(words, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300, env=full)
    assert done.returncode == 0, "api_stages %s ended with %d: %s%s" % (" ".join(words[2:]), done.returncode, done.stdout[-2000:], done.stderr[-2000:])
    return done.stdout


def triple(v):
    """x,y,z of binary32 values in a text that reads back exactly"""
    return ",".join("%.9g" % np.float32(x) for x in v)


def write(path, array):
    np.ascontiguousarray(array).tofile(str(path))
    return str(path)


def read(outdir, name, dtype):
    return np.fromfile(os.path.join(str(outdir), name), dtype=dtype)


def speaker_records(speakers):
    """[(direction, coefficient)] -> Speaker records"""
    s = aligned_zeros(len(speakers), SPEAKER)
    for i, (direction, k) in enumerate(speakers):
        s["direction"][i, :3] = direction
        s["coefficient"][i] = k
    return s


def same_bits(got, want):
    """Equal bit patterns of two record (or float) arrays; where the oracle has a NaN any NaN will do (its payload is open)."""
    g = np.ascontiguousarray(got).reshape(-1).view(np.uint32)
    w = np.ascontiguousarray(want).reshape(-1).view(np.uint32)
    if g.shape != w.shape:
        return False
    differ = g != w
    if not differ.any():
        return True
    return bool((np.isnan(g.view(np.float32)[differ]) & np.isnan(w.view(np.float32)[differ])).all())


def first_difference(got, want):
    """For a failure message: the first record that differs, as both sides read it"""
    if got.shape != want.shape:
        return "%d records, the oracle has %d" % (got.shape[0], want.shape[0])
    g = np.ascontiguousarray(got).view(np.uint32).reshape(got.shape[0], -1)
    w = np.ascontiguousarray(want).view(np.uint32).reshape(want.shape[0], -1)
    bad = np.flatnonzero((g != w).any(axis=1))
    return "%d of %d records differ, the first at %d: got %r, the oracle has %r" % (bad.size, got.shape[0], bad[0], got[bad[0]], want[bad[0]])


def live(records):
    """records (raw or attenuated) that carry volume"""
    return (records["volume"] != 0).any(axis=1)


# ---- the oracle's answer for the stages behind attenuate ------------------------------------------------------------------------------

def oracle_attenuate(oracle, mic, records, model):
    """model: {"speakers": [(direction, coefficient)]} or {"hrtf": table [2][360][180][8], "facing":, "up":}"""
    if "speakers" in model:
        return [oracle.attenuate_speaker(mic, records, d, k) for d, k in model["speakers"]]
    return [oracle.attenuate_hrtf(mic, records, model["hrtf"][ear], model["facing"], model["up"], ear) for ear in (0, 1)]


def oracle_later_stages(oracle, attenuated, rate, per_channel=False):
    """What api_stages.cpp writes behind attenuated_c.bin, by the oracle and on copies: {"flat_raw": [c] of [8][bins], "predelay": [1] or
    [channels] floats, "fixed": [c] records, "flat": [c] of [8][bins]}."""
    out = {"flat_raw": [oracle.flatten(a, rate) for a in attenuated], "fixed": [a.copy() for a in attenuated]}
    if per_channel:
        pd = [oracle.find_predelay([a]) for a in attenuated]
    else:
        pd = [oracle.find_predelay(attenuated)] * len(attenuated) if attenuated else []
    for a, seconds in zip(out["fixed"], pd):
        oracle.fix_predelay(a, seconds)
    out["predelay"] = np.asarray(pd if per_channel else pd[:1], np.float32)
    out["flat"] = [oracle.flatten(a, rate) for a in out["fixed"]]
    return out


def crowded_bins(attenuated, rate):
    """bins that receive more than one live record"""
    a = attenuated[live(attenuated)]
    bins = np.round(a["time"].astype(np.float32) * np.float32(rate)).astype(np.int64)
    return int(np.count_nonzero(np.bincount(bins) > 1)) if bins.size else 0


def assert_later_stages(outdir, attenuated, want, what):
    """attenuated_c, flat_raw_c, predelay, fixed_c and flat_c of one run against the oracle's"""
    n = len(attenuated)
    for c in range(n):
        got = read(outdir, "attenuated_%d.bin" % c, ATTENUATED)
        assert same_bits(got, attenuated[c]), "%s: attenuated channel %d: %s" % (what, c, first_difference(got, attenuated[c]))
    assert not os.path.exists(os.path.join(str(outdir), "attenuated_%d.bin" % n)), what + ": more channels than the model has"
    got = read(outdir, "predelay.bin", np.float32)
    assert got.shape == want["predelay"].shape and (got == want["predelay"]).all(), "%s: findPredelay %r, the oracle has %r" % (what, got, want["predelay"])
    for c in range(n):
        got = read(outdir, "fixed_%d.bin" % c, ATTENUATED)
        assert same_bits(got, want["fixed"][c]), "%s: fixPredelay, channel %d: %s" % (what, c, first_difference(got, want["fixed"][c]))
        for stem in ("flat_raw", "flat"):
            flat = read(outdir, "%s_%d.bin" % (stem, c), np.float32)
            w = want[stem][c]
            assert flat.size == w.size, "%s: %s, channel %d: %d samples per band, the oracle has %d" % (what, stem, c, flat.size // 8, w.shape[1])
            if not same_bits(flat, w):
                band, bin_ = np.argwhere(flat.reshape(w.shape).view(np.uint32) != w.view(np.uint32))[0]
                raise AssertionError("%s: %s, channel %d, band %d, bin %d: got %r, the oracle has %r" % (
                    what, stem, c, band, bin_, flat.reshape(w.shape)[band, bin_], w[band, bin_]))


# ---- degenerate vectors ------------------------------------------------------------------------------------------------------------------

BIG = 2 * THREAD_THRESHOLD                  # with RVB_HOST_THREADS=8: eight ranges of 16 384


def _filled(n, seed):
    """n records of seeded non-zero volumes and positions 2 .. 12 m from the origin, all times zero"""
    rng = np.random.default_rng(seed)
    rec = aligned_zeros(n, IMPULSE)
    d = rng.normal(size=(n, 3))
    rec["position"][:, :3] = (d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(2.0, 12.0, (n, 1))).astype(np.float32)
    rec["volume"] = (rng.uniform(0.1, 1.0, (n, 8)) * rng.choice([-1.0, 1.0], (n, 8))).astype(np.float32)
    return rec


def degenerate_times():
    """name -> times [n] float32 of the degenerate vectors (no NaN and no negative time: the reference's flattenImpulses is undefined
    for them).  The two `big_` vectors have BIG elements: with eight host threads seven ranges hold no non-zero time."""
    t = {"empty": np.zeros(0, np.float32), "one": np.array([0.013], np.float32), "zero_times": np.zeros(300, np.float32)}
    t["last_only"] = np.zeros(1000, np.float32)
    t["last_only"][-1] = 0.25
    t["big_last_only"] = np.zeros(BIG, np.float32)
    t["big_last_only"][-1] = 0.25
    t["big_first_of_last_range"] = np.zeros(BIG, np.float32)
    t["big_first_of_last_range"][BIG - BIG // 8] = 0.25
    rng = np.random.default_rng(404)
    mixed = rng.uniform(0.002, 0.02, 200).astype(np.float32)
    mixed[::3] = np.float32(-0.0)                            # the first and the last element among them
    mixed[-1] = np.float32(-0.0)
    t["negative_zeros"] = mixed
    return t


def degenerate_records():
    """name -> impulse records with the times of degenerate_times() and live volumes, and `zero_volumes`: non-zero times, no volume
    (every record attenuates to {0, 0})."""
    out = {}
    for i, (name, times) in enumerate(sorted(degenerate_times().items())):
        rec = _filled(times.shape[0], 50 + i)
        rec["time"] = times
        out[name] = rec
    rec = _filled(50, 49)
    rec["volume"] = 0
    rec["time"] = np.random.default_rng(48).uniform(0.002, 0.02, 50).astype(np.float32)
    out["zero_volumes"] = rec
    return out
