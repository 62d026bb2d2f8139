"""The cases and the binary64 reference of the source-end gradients (include/rvb_capi_source_grad.h), shared by
tests/test_gpu_source_grad.py and tests/test_source_grad_cases_host.py.  Everything here runs on the CPU.

The reference is built from things other tests pin bit for bit: the CPU oracle's trace of a case with NO directivity is the kept
trace's unscaled records (tests/test_gpu_parity.py, test_gpu_reshade.py, test_gpu_relisten.py hold the GPU's records, re-shaded or
re-listened, to it), the oracle's attenuate_speaker is the materialised speaker attenuation, bins_of the binary32 time_bin.  With
term[i][b] = sum_c w[c][b][bin_i] * att_c.volume[i][b] (state_terms of tests/test_gpu_reshade_grad.py)
    Lambda_ref[r][b] = sum over the records i of ray r of term[i][b],     A[r][b] the same over |term|,
and the same per image of the oracle's merged list.  The bar, the family's derived one:  |gpu - ref| <= 4 (nreflections + 16) 2^-24 A +
1e-30 entry by entry — the same count of roundings covers these terms, which are rvb_reshade_grad's with one factor fewer.  For the
pattern gradient, with u = normalize3(normalize3(v)) and d = dot3(u, n) redone here in binary32,
    shape_ref[b] = sum Lambda_ref (d - 1),   direction_ref[j] = sum (sum_b shape_b Lambda_ref) u_j
and the same bar with A weighted by |d - 1| or shape_b |u_j| and 4 more roundings (two normalisations, the dot, the difference).

The ground condition (assert_ground) is asserted on the reference alone, before any comparison: a gradient of rounding noise must not
pass.  The weight seeds below were picked so that every case satisfies it; tests/test_source_grad_cases_host.py holds that on the CPU."""
import numpy as np

from parallel_reverb_raytracer_amd import scenes
from parallel_reverb_raytracer_amd.dtypes import AIR_COEFFICIENTS, aligned_copy

from test_gpu_reshade import AIR_B, SPEAKERS
from test_gpu_reshade_grad import bins_of, state_terms, table_t, weights
from test_gpu_source_pattern import FACING, SHAPES

SR = 44100.0
F32 = np.float32
MIC, SRC = (0.5, 1.0, 2.0), (-0.7, -1.2, -3.0)
OTHER_MIC = (-1.0, 2.0, -1.5)                   # after a relisten; the microphone of pair 1
OTHER_SRC = (0.9, -2.0, 1.0)                    # the source of pair 1
TABLE_SEED = 11

RAYS = (1, 7, 8, 9, 65)                         # the edges of 8 rays per wave and of a wave
REFLECTIONS = (1, 15, 16, 17, 33)               # the edges of GRAD_TILE


def room(open_wall=False):
    """scenes.shoebox(4, 7, 10): twelve triangles, specular walls — every ray has images.  open_wall: without its last two triangles (one
    wall), so that rays leave the room."""
    triangles, vertices, surfaces = scenes.shoebox(4.0, 7.0, 10.0)
    return (aligned_copy(triangles[:-2]) if open_wall else triangles, vertices, surfaces)


def case(name, nrays, nrefl, seed, **more):
    c = {"name": name, "nrays": nrays, "nrefl": nrefl, "seed": seed, "open": False, "table": None, "air": AIR_COEFFICIENTS, "mic": MIC, "src": SRC,
         "half_bins": False, "late_predelay": False, "dead_band": None, "axis_rays": False, "direction": FACING, "shapes": SHAPES, "dir_seed": 23}
    c.update(more)
    return c


# (name, rays, reflections, weight seed) — the seeds: see the module text
SHAPE_CASES = [case("%dx%d" % (nrays, nrefl), nrays, nrefl, seed)
               for (nrays, nrefl), seed in zip([(r, k) for r in RAYS for k in REFLECTIONS],
                                               [5, 5, 5, 5, 5, 5, 5, 6, 5, 6, 5, 5, 5, 5, 5, 5, 5, 6, 5, 5, 5, 5, 5, 5, 6])]
ESCAPES = case("escaping rays", 65, 17, 5, open=True)
HALF_BINS = case("nbins cuts late records off", 65, 17, 6, half_bins=True)
PREDELAY = case("a predelay", 65, 17, 5, late_predelay=True)
DEAD_BAND = case("a zero specular coefficient in band 3", 65, 17, 5, dead_band=3, table=TABLE_SEED)
RESHADED = case("after a reshade to another table", 65, 17, 5, table=TABLE_SEED, air=AIR_B)
RELISTENED = case("after a relisten", 65, 17, 5, mic=OTHER_MIC)
PAIR_1 = case("pair 1 of two", 65, 17, 5, mic=OTHER_MIC, src=OTHER_SRC)
NULL = case("rays at a null of the pattern", 70, 17, 6, axis_rays=True, direction=(0.0, 0.0, 1.0), shapes=(0.25, 0.5, 1.0, 0.75, 1.0, 0.3, 0.6, 0.9))
EDGE_CASES = [ESCAPES, HALF_BINS, PREDELAY, DEAD_BAND, RESHADED, RELISTENED, PAIR_1, NULL]

AXES = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1)], F32)


def directions_of(c):
    """[nrays][4] float32: the seeded stream; axis_rays: its first five replaced by axis-aligned directions, four of them at right angles
    to (0, 0, 1) — d == 0 exactly, in binary32 — and one along it"""
    d = scenes.sphere_directions(c["nrays"], seed=c["dir_seed"]).copy()
    if c["axis_rays"]:
        d[:5, :3] = AXES
    return d


def table_of(c, surfaces):
    """The surface table of the case: the scene's own, or the seeded other one, with a zero specular coefficient in the dead band"""
    t = aligned_copy(surfaces) if c["table"] is None else table_t(surfaces, seed=c["table"])
    if c["dead_band"] is not None:
        t["specular"][:, c["dead_band"]] = 0.0
    return t


def unit_twice(v):
    """normalize3(normalize3(v)) of csrc/rvb_math.h in binary32, row by row: x*x + y*y + z*z left to right, sqrtf, three divisions; a zero
    vector stays zero"""
    v = np.asarray(v, F32).reshape(-1, 3).copy()
    for _ in range(2):
        x, y, z = v[:, 0], v[:, 1], v[:, 2]
        length = np.sqrt((x * x + y * y) + z * z).astype(F32)
        safe = np.where(length == 0, F32(1.0), length)
        v = np.where(length[:, None] == 0, v, (v / safe[:, None]).astype(F32)).astype(F32)
    return v


def pattern_geometry(vectors, direction):
    """(u [n][3], d [n]) in binary32 as the gain takes them; the pattern's direction is normalised once on the host"""
    n = np.asarray(direction, F32).reshape(1, 3)
    length = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]).astype(F32)
    n = (n / length[:, None]).astype(F32)[0]
    u = unit_twice(vectors)
    d = ((u[:, 0] * n[0] + u[:, 1] * n[1]).astype(F32) + u[:, 2] * n[2]).astype(F32)
    return u, d


def gains_of(shapes, d):
    """g[n][8] = (1 - shape) + shape * d in binary32 (band_gain of csrc/attenuation.h)"""
    s = np.broadcast_to(np.asarray(shapes, F32).reshape(-1), (8,))
    return ((F32(1.0) - s)[None, :] + (s[None, :] * d[:, None]).astype(F32)).astype(F32)


def binning_of(c, diffuse, images):
    """(predelay, nbins) of the case from the unscaled records: the first arrival and the bins up to the last — or a predelay behind the
    sixth live record, at least five samples late, so that several records clamp to bin 0 — or half the bins, so that late records are
    skipped"""
    live = (diffuse["volume"] != 0).any(axis=1)
    times = np.concatenate([diffuse["time"][live], images["time"][(images["volume"] != 0).any(axis=1)]]).astype(F32)
    times = times[times > 0]
    lo, hi = F32(times.min()), F32(times.max())
    predelay = lo
    if c["late_predelay"]:
        predelay = max(F32(lo + F32(5.0 / SR)), np.sort(diffuse["time"][live])[5])
    nbins = int(bins_of([hi], predelay, SR)[0]) + 1
    if c["half_bins"]:
        nbins //= 2
    return float(predelay), nbins


_references = {}


def reference(oracle, c):
    """Everything the comparisons of case `c` need, from the oracle alone.  Computed once per case and never changed."""
    if c["name"] in _references:
        return _references[c["name"]]
    scene = room(c["open"])
    table = table_of(c, scene[2])
    dirs = directions_of(c)
    nrays, nrefl = c["nrays"], c["nrefl"]
    diffuse, image, index = oracle.raytrace((scene[0], scene[1], table), c["mic"], c["src"], dirs, nrefl, c["air"])
    images = oracle.collect_images(image, index, False)
    predelay, nbins = binning_of(c, diffuse, images)
    w = weights(len(SPEAKERS[1]), nbins, c["seed"])
    scale = 4.0 * (nrefl + 16) * 2.0 ** -24
    pattern_scale = 4.0 * (nrefl + 20) * 2.0 ** -24
    r = {"case": c, "scene": scene, "table": table, "dirs": dirs, "predelay": predelay, "nbins": nbins, "w": w, "diffuse": diffuse, "images": images}
    term, absterm, _, bins, _ = state_terms(oracle, c["mic"], SPEAKERS, predelay, SR, nbins, w, diffuse)
    r["lambda"] = term.reshape(nrays, nrefl, 8).sum(axis=1)
    r["a"] = absterm.reshape(nrays, nrefl, 8).sum(axis=1)
    r["bar"] = scale * r["a"] + 1e-30
    r["live_rays"] = (diffuse["volume"] != 0).any(axis=1).reshape(nrays, nrefl).any(axis=1)
    r["bins"] = bins
    term, absterm, _, image_bins, _ = state_terms(oracle, c["mic"], SPEAKERS, predelay, SR, nbins, w, images)
    r["image_lambda"], r["image_a"], r["image_bar"], r["image_bins"] = term, absterm, scale * absterm + 1e-30, image_bins
    # the pattern gradient of the diffuse part and of the image part
    for part, vectors, lam, a in (("rays_pattern", dirs[:, :3], r["lambda"], r["a"]),
                                  ("images_pattern", (np.asarray(c["mic"], F32)[None, :] - images["position"][:, :3]).astype(F32), r["image_lambda"], r["image_a"])):
        u, d = pattern_geometry(vectors, c["direction"])
        u64, d1 = u.astype(np.float64), d.astype(np.float64) - 1.0
        s = np.broadcast_to(np.asarray(c["shapes"], F32).reshape(-1), (8,)).astype(np.float64)
        along, along_a = (lam * s[None, :]).sum(axis=1), (a * s[None, :]).sum(axis=1)
        r[part] = {"u": u, "d": d, "gains": gains_of(c["shapes"], d),
                   "shape": (lam * d1[:, None]).sum(axis=0), "shape_bar": pattern_scale * (a * np.abs(d1)[:, None]).sum(axis=0) + 1e-30,
                   "direction": (along[:, None] * u64).sum(axis=0), "direction_bar": pattern_scale * (along_a[:, None] * np.abs(u64)).sum(axis=0) + 1e-30}
    _references[c["name"]] = r
    return r


def assert_ground(r):
    """On the reference alone: A > 0 for every ray with a live record (but in the band a zero coefficient ends), at least half of the
    (ray, band) entries and every entry of the rays' pattern gradient stand 100 bars clear of zero."""
    c = r["case"]
    bands = np.arange(8) != (-1 if c["dead_band"] is None else c["dead_band"])
    assert r["live_rays"].any(), c["name"]
    inside = r["live_rays"] & (r["a"] > 0).any(axis=1)              # (a ray whose live records all lie past the histogram adds nothing)
    assert inside.any() and (r["a"][inside][:, bands] > 0).all(), c["name"]
    clear = np.abs(r["lambda"]) >= 100.0 * r["bar"]
    assert clear.mean() >= 0.5, (c["name"], clear.mean())
    assert (np.abs(r["rays_pattern"]["shape"])[bands] >= 100.0 * r["rays_pattern"]["shape_bar"][bands]).all(), (c["name"], np.abs(r["rays_pattern"]["shape"]) / r["rays_pattern"]["shape_bar"])
    assert (np.abs(r["rays_pattern"]["direction"]) >= 100.0 * r["rays_pattern"]["direction_bar"]).all(), (c["name"], np.abs(r["rays_pattern"]["direction"]) / r["rays_pattern"]["direction_bar"])


def assert_image_ground(r):
    """The same for the image part: at least half of the (image, band) entries of the live images, and every entry of their pattern
    gradient, stand 100 bars clear of zero."""
    c = r["case"]
    live = r["image_a"].any(axis=1)
    assert live.sum() >= 3, c["name"]
    clear = np.abs(r["image_lambda"][live]) >= 100.0 * r["image_bar"][live]
    assert clear.mean() >= 0.5, (c["name"], clear.mean())
    assert (np.abs(r["images_pattern"]["shape"]) >= 100.0 * r["images_pattern"]["shape_bar"]).all(), (c["name"], np.abs(r["images_pattern"]["shape"]) / r["images_pattern"]["shape_bar"])
    assert (np.abs(r["images_pattern"]["direction"]) >= 100.0 * r["images_pattern"]["direction_bar"]).all(), (c["name"], np.abs(r["images_pattern"]["direction"]) / r["images_pattern"]["direction_bar"])
