"""The owner of the mirror's opt-in device-resident handover (parallel-reverb-raytracer_amd/host/resident_cache.h) alone:
tests/cpp/resident_cache.cpp, which includes nothing else of the library, is compiled as C++11 host code with AddressSanitizer and
UndefinedBehaviorSanitizer into a temporary directory and run once; what it printed is held against the values below, which are
written out from the contract in INTEGRATION.md (the RVB_API_RESIDENT row) and the banner comment of the header.  "Device copies"
are malloc'ed blocks under a counting deleter; `freed` is how often a deleter has run when the step ends.  No GPU, nothing loaded
into Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "parallel-reverb-raytracer_amd", "host")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SANITIZE = "-fsanitize=address,undefined"
N = 600                     # elements of 16 bytes per vector: stride 251 samples 0, 251, 502 and the last, 599


@pytest.fixture(scope="module")
def steps(tmp_path_factory):
    tool = os.path.join(str(tmp_path_factory.mktemp("resident_cache")), "resident_cache")
    subprocess.check_call([HIPCC, "-x", "c++", "-std=c++11", "-O1", "-g", "-Wall", SANITIZE, "-fno-sanitize-recover=all", "-I" + HOST,
                           os.path.join(ROOT, "tests", "cpp", "resident_cache.cpp"), "-o", tool])
    done = subprocess.run([tool], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=120)
    print(done.stdout)
    assert done.returncode == 0 and done.stderr == "", done.stderr           # a sanitizer report goes to stderr and ends the program
    got = {}
    for line in done.stdout.splitlines():
        words = line.split()
        assert words[0] not in got, line
        got[words[0]] = {k: int(v) for k, v in (item.split("=", 1) for item in words[1:])}
    return got


def nothing(freed):
    """find() answered false"""
    return {"found": 0, "device_count": 0, "owned": 0, "lease": 0, "device_ok": 1, "freed": freed}


def owned(freed):
    """find() handed out the right owned copy of the whole vector, with a reference for the reader"""
    return {"found": 1, "device_count": N, "owned": 1, "lease": 1, "device_ok": 1, "freed": freed}


def borrowed(freed, device_count=N):
    """find() handed out the owner's trace buffer: no reference goes with it"""
    return {"found": 1, "device_count": device_count, "owned": 0, "lease": 0, "device_ok": 1, "freed": freed}


def pick(steps, names):
    assert set(names) <= set(steps), sorted(set(names) - set(steps))
    return {name: steps[name] for name in names}


def test_the_program_includes_the_cache_header_alone():
    with open(os.path.join(ROOT, "tests", "cpp", "resident_cache.cpp")) as f:
        local = [l.split('"')[1] for l in f if l.startswith('#include "')]
    assert local == ["resident_cache.h"]
    with open(os.path.join(HOST, "resident_cache.h")) as f:
        text = f.read()
    assert not [l for l in text.splitlines() if l.startswith('#include "') or (l.startswith("#include") and "hip/" in l)]
    assert "getenv" not in text and "rvb_capi" not in text and "class ResidentCache" in text


def test_finding_and_keys(steps):
    """"a vector this library returned is then recognised when it comes back (buffer address, length ...)": the key is (address,
    count, element size); another address leaves the entry alone, another count or element size at ITS address drops it"""
    want = {
        "fresh": nothing(0),
        "null_host": nothing(0),
        "remembered": owned(0),
        "other_address": nothing(0),
        "other_address_then_right_key": owned(0),
        "other_count": nothing(1),                       # dropped: the deleter ran once ...
        "other_count_then_right_key": nothing(1),        # ... and the right key finds nothing any more
        "other_elem": nothing(2),                        # (remembered again in between)
        "other_elem_then_right_key": nothing(2),
    }
    assert pick(steps, want) == want


def test_edits_and_samples(steps):
    """"a sample of every 251st element" and the last; "an in-place edit that misses every sampled element is NOT seen in that
    mode, which is why it is not the default" """
    want = {
        "edit_0": nothing(3), "edit_0_then_again": nothing(3),
        "edit_251": nothing(4), "edit_251_then_again": nothing(4),
        "edit_599": nothing(5), "edit_599_then_again": nothing(5),
        "edit_1_unseen": owned(5),                       # the documented hole: nobody "fixes" it silently
        "edit_251_then_resample": owned(5),              # fixPredelay edits vector and copy alike, then resamples
    }
    assert pick(steps, want) == want


def test_replacement_and_eviction(steps):
    """a buffer address names one vector at a time; owned copies are kept up to the byte cap (here 20000: two copies of 9600 bytes
    fit, three do not), oldest dropped first; borrowed entries neither count nor go"""
    want = {
        "replaced": owned(6),                            # the old copy's deleter ran, the new copy is handed out
        "two_owned_one_borrowed_a": owned(6),            # 19200 owned + 9600 borrowed bytes: nothing evicted
        "third_owned_a": nothing(7),                     # the oldest owned copy went ...
        "third_owned_b": {"found": 1, "freed": 7},       # ... and it alone
        "third_owned_c": {"found": 1, "freed": 7},
        "third_owned_borrowed": borrowed(7),
        "evict_0": {"answer": 1, "freed": 9},
        "evict_0_b": {"found": 0, "freed": 9},
        "evict_0_c": {"found": 0, "freed": 9},
        "evict_0_borrowed": borrowed(9),
        "evict_0_again": {"answer": 0, "freed": 9},
    }
    assert pick(steps, want) == want


def test_a_reader_keeps_its_copy_alive(steps):
    """the lease: evicting or replacing an entry lets go of the cache's reference only; the deleter runs when the reader is done"""
    want = {
        "lease_evicted": {"answer": 1, "freed": 9},      # the entry went, the deleter has not run ...
        "lease_evicted_block": {"readable": 1, "freed": 9},
        "lease_evicted_then_find": nothing(9),
        "lease_evicted_then_dropped": {"answer": 1, "freed": 10},        # ... until the reader let go: once
        "lease_replaced_block": {"readable": 1, "freed": 10},
        "lease_replaced_then_find": owned(10),           # the replacement, not the reader's copy
        "lease_replaced_then_dropped": {"answer": 1, "freed": 11},
    }
    assert pick(steps, want) == want


def test_owners_and_stamps(steps):
    """"the context's trace generation": a borrowed entry (the leading 500 elements here) is void once its owner traces again,
    also when the owner's count was read before that trace and the entry made after it"""
    want = {
        "borrowed": borrowed(11, 500),
        "owner_1_traced_its_borrowed": nothing(11),
        "owner_1_traced_other_borrowed": borrowed(11, 500),
        "owner_1_traced_owned": owned(11),
        "stale_stamp": nothing(11),
        "fresh_stamp": borrowed(11, 500),
    }
    assert pick(steps, want) == want


def test_cache_off(steps):
    """the default: nothing is remembered; an owned copy is let go at once"""
    want = {"off_owned": nothing(12), "off_borrowed": nothing(12)}
    assert pick(steps, want) == want


def test_every_deleter_ran_once(steps):
    """15 blocks were made; the three the caches still hold at the end (the unseen edit's, the lease replacement, the owners' owned
    copy) have not been freed, every other one exactly once; and no step went unchecked"""
    assert steps["end"] == {"made": 15, "once": 12, "more": 0, "held": 3, "freed": 12}
    assert len(steps) == 9 + 8 + 11 + 7 + 6 + 2 + 1                   # the tests above, in their order, and "end"
