"""The cases of tests/test_gpu_source_grad.py on the CPU (tests/source_grad_cases.py): every case's reference, built from the oracle
alone, satisfies the ground condition with its committed weight seed — entries that stand clear of rounding noise —, the constructed
edges are there (escaping rays, records past the histogram, records clamped to bin 0, a dead band, rays at an exact null of the
pattern), and the binary32 restatement of the pattern's gain equals the oracle's attenuate_speaker on a departure vector."""
import numpy as np
import pytest

import source_grad_cases as S
from parallel_reverb_raytracer_amd.dtypes import IMPULSE, aligned_zeros


@pytest.mark.parametrize("case", S.SHAPE_CASES + S.EDGE_CASES, ids=[c["name"] for c in S.SHAPE_CASES + S.EDGE_CASES])
def test_the_reference_of_every_case_stands_clear_of_rounding_noise(oracle, case):
    r = S.reference(oracle, case)
    S.assert_ground(r)
    if case["nrays"] >= 65:
        S.assert_image_ground(r)


def test_the_edges_are_in_the_cases(oracle):
    r = S.reference(oracle, S.ESCAPES)
    assert (~r["live_rays"]).sum() >= 5 and r["live_rays"].sum() >= 30 and not r["a"][~r["live_rays"]].any()
    r = S.reference(oracle, S.HALF_BINS)
    live = (r["diffuse"]["volume"] != 0).any(axis=1)
    assert (live & (r["bins"] >= r["nbins"])).sum() >= 50 and (live & (r["bins"] < r["nbins"])).sum() >= 50
    r = S.reference(oracle, S.PREDELAY)
    live = (r["diffuse"]["volume"] != 0).any(axis=1)
    clamped = live & (r["diffuse"]["time"] <= np.float32(r["predelay"]))
    assert clamped.sum() >= 3 and (r["bins"][clamped] == 0).all()
    r = S.reference(oracle, S.DEAD_BAND)
    assert not r["a"][:, 3].any() and (r["a"][r["live_rays"]][:, [0, 1, 2, 4, 5, 6, 7]] > 0).all()
    r = S.reference(oracle, S.NULL)
    at_null = r["rays_pattern"]["d"][:4] == 0
    assert at_null.all() and not r["rays_pattern"]["gains"][:4][:, [2, 4]].any(), "no ray stands at an exact null of bands 2 and 4"
    assert (np.abs(r["lambda"][:4][:, [2, 4]]) >= 100.0 * r["bar"][:4][:, [2, 4]]).all(), "the derivative at the null is not clear of zero"


def test_the_binary32_gain_is_the_oracles(oracle):
    """g_b of the pattern's CONTRACT is the reference's `attenuate` fed with a departure vector: fake microphone 0, fake position = v"""
    c = S.SHAPE_CASES[-1]
    dirs = S.directions_of(c)
    u, d = S.pattern_geometry(dirs[:, :3], c["direction"])
    gains = S.gains_of(c["shapes"], d)
    fake = aligned_zeros(dirs.shape[0], IMPULSE)
    fake["volume"] = 1.0
    fake["position"][:, :3] = dirs[:, :3]
    for b in range(8):
        want = oracle.attenuate_speaker((0.0, 0.0, 0.0), fake, c["direction"], float(np.float32(c["shapes"][b])))["volume"][:, b]
        assert np.array_equal(gains[:, b], want), b
