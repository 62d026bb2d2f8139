"""The constructed inputs of tests/attenuation_edges.py, held against the CPU oracle alone (no GPU): before
tests/test_gpu_attenuation_edges.py feeds them to the kernels, they must put the features under test — both neighbours of every
integer-degree boundary, angles inside the claimed atan2f error and outside the fallback margin of csrc/attenuation.h (angle_deg),
the quirk rows, exact half bins, and a fast-mode table under which a neighbouring row cannot hide inside the rounding bound."""
import numpy as np
import pytest

import attenuation_edges as ae
from test_gpu_speaker_arrays import fast_bound

FRAMES = {"canonical": ae.CANONICAL, "oblique": ae.OBLIQUE}


@pytest.fixture(scope="module")
def sweeps(oracle):
    """Per frame: the records, the builder's dict, the oracle's row of every record and the binary64 angles of the stored positions."""
    out = {}
    table = ae.row_code_table()
    for name, fr in FRAMES.items():
        rec, b, names = ae.boundary_set(fr)
        att = oracle.attenuate_hrtf(fr["mic"], rec, table[0], fr["facing"], fr["up"], 0)
        az, el = ae.listener_angles(fr["facing"], fr["up"], fr["mic"], rec["position"][:, :3])
        out[name] = {"rec": rec, "b": b, "names": names, "row": ae.rows_from_codes(att["volume"]), "az": az, "el": el,
                     "n": b["position"].shape[0]}
    return out


def _signed_distance(s):
    """Binary64 distance of every sweep record's swept angle from its boundary k, in degrees (azimuth: across the wrap)."""
    n, b = s["n"], s["b"]
    is_az = b["kind"] == "az"
    d_az = (s["az"][:n] + 180.0 - b["k"] + 180.0) % 360.0 - 180.0
    d_el = s["el"][:n] - b["k"]
    return np.where(is_az, d_az, d_el), is_az


def test_the_sweep_has_about_eighty_thousand_records(sweeps):
    for s in sweeps.values():
        assert 79000 <= s["n"] <= 81000
        assert s["rec"].shape[0] == s["n"] + len(s["names"])
        assert (s["rec"]["time"] >= 1e-3).all() and (s["rec"]["volume"] == 1).all()


@pytest.mark.parametrize("frame", list(FRAMES))
def test_both_neighbours_of_every_boundary_are_among_the_oracles_rows(sweeps, frame):
    s = sweeps[frame]
    n, b, row = s["n"], s["b"], s["row"][:s["n"]]
    a, e = row // 180, row % 180            # (e == 180 shows as the next azimuth's e == 0, quirk Q5: not at these elevations)
    have_az, have_el = 0, 0
    for k in range(1, 360):
        got = set(a[(b["kind"] == "az") & (b["k"] == k)].tolist())
        assert {k - 1, k} <= got, (frame, "az", k, sorted(got))
        have_az += 1
    for k in list(range(-89, 0)) + list(range(1, 90)):
        # the elevation truncates toward zero: boundary k separates trunc = k from trunc = k - sign(k); k = 0 is no boundary
        sel = (b["kind"] == "el") & (b["k"] == k)
        got = set((90 - e[sel]).tolist())
        assert {k, k - int(np.sign(k))} <= got, (frame, "el", k, sorted(got))
        have_el += 1
    assert (have_az, have_el) == (359, 178)
    sel0 = (b["kind"] == "el") & (b["k"] == 0)
    assert set(e[sel0].tolist()) == {90}, "-1 < el < 1 is one row"


@pytest.mark.parametrize("frame", list(FRAMES))
def test_every_boundary_has_angles_inside_the_claimed_error_and_outside_the_margin(sweeps, frame):
    """Both code paths of angle_deg run on every boundary: binary64 angles of the STORED binary32 positions within 1.2e-4 degrees
    (where a wrong error bound for atan2f would show) and beyond 2e-3 degrees (where the binary32 atan2f decides alone)."""
    s = sweeps[frame]
    dist, is_az = _signed_distance(s)
    b = s["b"]
    near = np.abs(dist) <= ae.CLAIMED_ATAN2F_ERROR_DEG
    far = np.abs(dist) > ae.ANGLE_MARGIN_DEG
    worst_near, worst_far = 10 ** 9, 10 ** 9
    for kind, ks in (("az", range(0, 361)), ("el", range(-90, 91))):
        for k in ks:
            sel = (b["kind"] == kind) & (b["k"] == k)
            sides = [+1] if (kind, k) == ("el", -90) else [-1] if (kind, k) == ("el", 90) else [-1, +1]      # the poles have one side
            for side in sides:
                on = sel & (np.sign(dist) == side)
                assert np.count_nonzero(on & near) >= 5, (frame, kind, k, side)
                assert np.count_nonzero(on & far) >= 2, (frame, kind, k, side)
                worst_near, worst_far = min(worst_near, np.count_nonzero(on & near)), min(worst_far, np.count_nonzero(on & far))
    share_inside_margin = np.mean(np.abs(dist) <= ae.ANGLE_MARGIN_DEG)
    print("%s: fewest records within 1.2e-4 deg per boundary side %d, beyond 2e-3 deg %d; %.1f %% of the swept angles inside the margin"
          % (frame, worst_near, worst_far, 100 * share_inside_margin))
    assert share_inside_margin > 0.8


def test_the_quirk_rows_appear(sweeps):
    can = sweeps["canonical"]
    for frame, s in sweeps.items():
        n, row = s["n"], s["row"]
        # Q5: e == 180 (elevation -90) runs into the next azimuth's row
        q5 = (s["b"]["kind"] == "el") & (s["b"]["k"] == -90) & (row[:n] % 180 == 0)
        assert np.count_nonzero(q5) >= 20, frame
        print("%s: %d records with e == 180" % (frame, np.count_nonzero(q5)))
        # a == 0 from both ends of the azimuth range: az = -180 + d, and az = +180 - d whose binary32 sum az + 180 rounds to 360
        a0 = (s["b"]["kind"] == "az") & (row[:n] // 180 == 0)
        assert np.count_nonzero(a0 & (s["az"][:n] < -179.0)) >= 10, frame
        assert np.count_nonzero(a0 & (s["az"][:n] > 179.0)) >= 3, frame
        assert np.count_nonzero((s["b"]["kind"] == "az") & (row[:n] // 180 == 359) & (s["az"][:n] > 179.0)) >= 10, frame
    # the padding row 360 * 180, and the named singles of the canonical frame (signed zeros exist only round a microphone at 0)
    single = dict(zip(can["names"], can["row"][can["n"]:].tolist()))
    assert single["padding_row"] == ae.HRTF_ROWS
    assert single["az_plus_180"] == 0 * 180 + 90 and single["az_minus_180"] == 0 * 180 + 90
    assert single["pole_north_x+0_z+0"] == 180 * 180 + 0
    assert single["pole_south_x+0_z+0"] == 180 * 180 + 180                   # Q5
    assert single["pole_south_x-0_z-0"] == 0 * 180 + 180                     # atan2(-0, -0) = -pi: the zeros' signs decide the row
    assert single["at_microphone"] == 180 * 180 + 90


@pytest.mark.parametrize("frame", list(FRAMES))
def test_oracle_rows_equal_binary64_rows_outside_the_margin(sweeps, frame):
    s = sweeps[frame]
    n = s["n"]
    az180, el = s["az"][:n] + 180.0, s["el"][:n]
    clear = (np.abs(az180 - np.rint(az180)) > ae.ANGLE_MARGIN_DEG) & (np.abs(el - np.rint(el)) > ae.ANGLE_MARGIN_DEG)
    assert np.count_nonzero(clear) > 5000
    want = (az180.astype(np.int64) % 360) * 180 + 90 - np.trunc(el).astype(np.int64)
    bad = np.flatnonzero(clear & (want != s["row"][:n]))
    assert bad.size == 0, [(ae.describe(s["b"], s["names"], i), int(want[i]), int(s["row"][i])) for i in bad[:5]]


def test_half_bins(oracle):
    """round(time * sample_rate) at products of exactly k + 0.5: at 44.1 kHz most k have such a binary32 time, with neighbours that
    round down and up; at the power-of-two rate every k has."""
    from parallel_reverb_raytracer_amd.dtypes import ATTENUATED, aligned_zeros
    for sr, need in ((44100.0, 2000), (8192.0, None)):
        rec, info = ae.time_edge_records(sr)
        k, t = info["half_k"], info["half_t"]
        prod = t * np.float32(sr)                                   # binary32, as the kernels and the oracle form it
        assert prod.dtype == np.float32
        exact = (prod == (k + 0.5)[:, None].astype(np.float32)).any(axis=1)
        both = (prod < (k + 0.5)[:, None]).any(axis=1) & (prod > (k + 0.5)[:, None]).any(axis=1)
        print("%g Hz: %d k kept, %d with an exact half bin, %d with neighbours on both sides" % (sr, k.size, exact.sum(), both.sum()))
        if need is None:
            assert exact.all() and both.all()
        else:
            assert exact.sum() >= need and both.sum() >= need
        # and the oracle rounds them half away from zero
        att = aligned_zeros(k.size, ATTENUATED)
        att["volume"] = 1
        att["time"] = t[:, 1]
        flat = oracle.flatten(att, sr)
        hit = prod[:, 1] == (k + 0.5).astype(np.float32)
        assert (flat[0][k[hit] + 1] >= 1).all()
        assert (rec["time"] >= np.float32(1e-3)).all()
        # the runs and the crowd sit where the builder says (no trim)
        bins = np.round(rec["time"] * np.float32(sr)).astype(np.int64)
        counts = np.bincount(bins[info["runs"]], minlength=info["run_bins"][-1] + 1)[info["run_bins"]]
        assert counts.tolist() == [1, 2, 3, 4, 5, 8, 9]
        assert set(bins[info["crowd"]].tolist()) == {info["crowd_bin"]}
        mags = np.abs(rec["volume"][info["crowd"]]).max(axis=1)
        assert (mags < 2e-3).sum() > 50 and ((mags > 0.1) & (mags < 1)).sum() > 50 and (mags > 3).sum() > 50
        assert rec["time"][0] == rec["time"].min() and np.count_nonzero(rec["time"] == rec["time"][0]) == 1


def test_fast_mode_table_separates_neighbouring_rows(oracle, sweeps):
    """Under spread_table() a record attenuated with a neighbouring row (a +- 1, e +- 1) moves its bin by more than four times the
    fast mode's rounding bound, in every band of both ears: a wrong row cannot pass the fast-mode test."""
    table = ae.spread_table()
    assert table.min() > 0 and table.max() <= 1
    flat_table = table.reshape(2, ae.HRTF_ROWS, 8).astype(np.float64)
    for frame, s in sweeps.items():
        fr = FRAMES[frame]
        chans = [oracle.attenuate_hrtf(fr["mic"], s["rec"], table[ch], fr["facing"], fr["up"], ch) for ch in (0, 1)]
        pd = oracle.find_predelay(chans)
        for c in chans:
            oracle.fix_predelay(c, pd)
        flats = [oracle.flatten(c, 44100.0) for c in chans]
        nb = max(f.shape[1] for f in flats)
        exact = np.zeros((2, 8, nb), np.float32)
        for ch in (0, 1):
            exact[ch][:, :flats[ch].shape[1]] = flats[ch]
        bound = fast_bound(exact, chans, 44100.0)
        live = s["row"] < ae.HRTF_ROWS
        rows = s["row"][live]
        for ch in (0, 1):
            bins = np.round(chans[ch]["time"][live] * np.float32(44100.0)).astype(np.int64)
            for other in ae.neighbour_rows(rows):
                moved = np.abs(flat_table[ch][other] - flat_table[ch][rows])            # unit volumes: [n][8]
                assert (moved > 4 * bound[ch][:, bins].T).all(), (frame, ch)


def test_speaker_edges_show_in_the_oracle(oracle):
    for mic in ((0.0, 0.0, 0.0), (1.0, 1.5, -2.0)):
        rec, names = ae.speaker_edge_records(mic)
        live = (rec["volume"] != 0).any(axis=1)
        assert np.count_nonzero(~live[7::8]) == rec[7::8].shape[0]
        out = {i: oracle.attenuate_speaker(mic, rec, d, c) for i, (d, c) in enumerate(ae.EDGE_SPEAKERS)}
        idx = {n: i for i, n in enumerate(names)}
        i = idx["on the speaker axis, dz=-2"]
        assert out[0]["volume"][i].tolist() == rec["volume"][i].tolist()                # coefficient 0: gain 1
        assert out[1]["volume"][i].tolist() == (-rec["volume"][i]).tolist()             # coefficient 1: gain -1
        assert not out[2]["volume"][i].any() and out[2]["time"][i] == rec["time"][i]    # 0.5: cancels to exactly 0, the time stays
        assert not out[3]["volume"][i].any()                                             # ... and with a direction of length 2
        i = idx["coordinates (3e+19, 3e+19, -3e+19)"]                                   # length3 overflows: the normal is 0, gain 1 - k
        assert out[4]["volume"][i].tolist() == (rec["volume"][i] * (np.float32(1) - np.float32(0.7))).tolist()
        i = idx["at the microphone"]
        assert out[8]["volume"][i].tolist() == (rec["volume"][i] * np.float32(0.0)).tolist()
        silent = [i for i, n in enumerate(names) if n == "volume -0.0 in all bands"]
        assert len(silent) >= 6 and all(out[0]["time"][i] == 0 for i in silent)
        kept = [i for i, n in enumerate(names) if n.startswith("volume -0.0 with band")]
        assert len(kept) >= 6 and all(out[0]["time"][i] == rec["time"][i] for i in kept)
        sub = [i for i, n in enumerate(names) if "subnormal volume" in n or n == "all bands subnormal"]
        tiny = np.finfo(np.float32).tiny
        assert sum(1 for i in sub if ((out[7]["volume"][i] != 0) & (np.abs(out[7]["volume"][i]) < tiny)).any()) >= 10
        if not any(mic):
            i = idx["offset (1e-25, -1e-25, 1e-25): squares underflow"]                 # length3 == 0, the vector is not: gain ~ 1 - k
            assert out[1]["volume"][i].any() and (np.abs(out[1]["volume"][i]) < 1e-20).all()
