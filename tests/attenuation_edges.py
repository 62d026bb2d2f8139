"""Builders of constructed edge inputs for the stages behind the trace: attenuation (speaker gain, HRTF table row, ear time shift),
predelay, time bin and the ordered / atomic folds.  A plain module: no fixtures, no GPU, no oracle — tests/test_attenuation_edge_inputs.py
checks with the CPU oracle that these inputs put the features under test, tests/test_gpu_attenuation_edges.py feeds them to the kernels.

Everything is built in binary64 and stored as binary32; every set is a pure function of its arguments (fixed seeds)."""
import numpy as np

from parallel_reverb_raytracer_amd.dtypes import IMPULSE, aligned_zeros

CANONICAL = {"facing": (0.0, 0.0, 1.0), "up": (0.0, 1.0, 0.0), "mic": (0.0, 0.0, 0.0), "radius": 1.0}
OBLIQUE = {"facing": (0.6, 0.0, 0.8), "up": (0.0, 1.0, 0.0), "mic": (1.0, 1.5, -2.0), "radius": 7.0}

HRTF_ROWS = 360 * 180                       # the padding row 360 * 180 follows them on the device

# distance of a constructed angle from its integer boundary, in degrees: 0 and 24 geometrically spaced magnitudes per sign
DELTA_MAGNITUDES = np.geomspace(2e-6, 4e-3, 24)
DELTAS = np.concatenate([[0.0], DELTA_MAGNITUDES, -DELTA_MAGNITUDES])

AZ_SWEEP_ELEVATIONS = (37.3, -61.7, 0.4)    # non-integer: the elevation of an azimuth-boundary record is never in doubt
EL_SWEEP_AZIMUTHS = (90.0, 33.6, -147.2)    # 90: t.z is the rounding residue of cos(90 deg), of either sign

CLAIMED_ATAN2F_ERROR_DEG = 1.2e-4           # csrc/attenuation.h, angle_deg: the bound the margin rests on
ANGLE_MARGIN_DEG = 2e-3                     # kAngleMargin


def listener_basis(facing, up):
    """The listener basis of the reference's transform (kernel.cpp:538-549) in binary64, from the binary32 values the kernels get:
    rows x = normalize(cross(up, facing)), y = cross(facing, x), z = facing."""
    f = np.asarray(facing, np.float32).astype(np.float64)
    u = np.asarray(up, np.float32).astype(np.float64)
    x = np.cross(u, f)
    x /= np.linalg.norm(x)
    return np.stack([x, np.cross(f, x), f])


def listener_angles(facing, up, mic, positions):
    """(azimuth, elevation) in degrees of binary32 positions, evaluated in binary64: what an exact evaluation of the kernels' two
    atan2 calls would give."""
    d = np.asarray(positions, np.float32).astype(np.float64) - np.asarray(mic, np.float32).astype(np.float64)
    t = d @ listener_basis(facing, up).T
    return np.degrees(np.arctan2(t[:, 0], t[:, 2])), np.degrees(np.arctan2(t[:, 1], np.hypot(t[:, 0], t[:, 2])))


def _directions(basis, az_deg, el_deg):
    """World directions whose listener-frame angles are (az, el): t = (sin az cos el, sin el, cos az cos el), d = basis^-1 t."""
    az, el = np.radians(az_deg), np.radians(el_deg)
    t = np.stack([np.sin(az) * np.cos(el), np.sin(el), np.cos(az) * np.cos(el)], -1)
    d = t @ np.linalg.inv(basis).T
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def hrtf_boundary_records(facing, up, mic, radius):
    """Positions whose true listener-frame angle sits at k + delta degrees, delta in DELTAS:
      * azimuth boundaries az + 180 = k, k = 0 .. 360 (0 and 360 are the wrap at -+180), at the elevations AZ_SWEEP_ELEVATIONS;
      * elevation boundaries k = -90 .. 90 (clipped to +-90: the poles), at the azimuths EL_SWEEP_AZIMUTHS.
    Returns a dict: position [n][3] float32, kind ('az' / 'el'), k, delta, other (the fixed angle of the sweep), and `singles`, named
    positions: the poles with every sign of the two zeros, az = +-180 exactly, the microphone itself, and a record whose elevation
    argument underflows (the padding row).  Signed zeros survive only where the microphone's coordinate is 0."""
    basis = listener_basis(facing, up)
    mic64 = np.asarray(mic, np.float32).astype(np.float64)
    kind, k_of, delta_of, other, az, el = [], [], [], [], [], []
    for e0 in AZ_SWEEP_ELEVATIONS:
        k, dl = np.meshgrid(np.arange(0, 361), DELTAS, indexing="ij")
        kind.append(np.full(k.size, "az")), k_of.append(k.ravel()), delta_of.append(dl.ravel()), other.append(np.full(k.size, e0))
        az.append((k - 180.0 + dl).ravel()), el.append(np.full(k.size, e0))
    for a0 in EL_SWEEP_AZIMUTHS:
        k, dl = np.meshgrid(np.arange(-90, 91), DELTAS, indexing="ij")
        kind.append(np.full(k.size, "el")), k_of.append(k.ravel()), delta_of.append(dl.ravel()), other.append(np.full(k.size, a0))
        az.append(np.full(k.size, a0)), el.append(np.clip(k + dl, -90.0, 90.0).ravel())
    az, el = np.concatenate(az), np.concatenate(el)
    position = (mic64 + radius * _directions(basis, az, el)).astype(np.float32)

    def at(d):
        """mic + radius * d with the sign of a zero kept where the microphone's coordinate is zero (x + 0 would lose it)."""
        d = np.asarray(d, np.float64) * radius
        return np.where(mic64 == 0.0, d, d + mic64).astype(np.float32)

    inv = np.linalg.inv(basis)
    canonical = np.array_equal(basis, np.eye(3))

    def frame(t):
        """listener-frame vector -> world; in the canonical frame the vector itself, zeros' signs included"""
        return np.asarray(t, np.float64) if canonical else inv @ np.asarray(t, np.float64)

    singles = {}
    for name, y in (("north", 1.0), ("south", -1.0)):
        for sx in (0.0, -0.0):
            for sz in (0.0, -0.0):
                singles["pole_%s_x%s_z%s" % (name, "-0" if np.signbit(sx) else "+0", "-0" if np.signbit(sz) else "+0")] = at(frame((sx, y, sz)))
    singles["az_plus_180"] = at(frame((0.0, 0.0, -1.0)))                 # t.x = +0, t.z < 0: atan2 = +pi
    singles["az_minus_180"] = at(frame((-0.0, -0.0, -1.0)))              # every term of t.x is -0: atan2 = -pi
    singles["at_microphone"] = np.asarray(mic, np.float32)
    # canonical frame: t.x = 1e-27, t.z = -1e-25, their squares underflow: el = atan2(-1, 0) = -90, e = 180, a = 359 -> row 64800
    singles["padding_row"] = at(frame((1e-27, -1.0, -1e-25)))
    return {"position": position, "kind": np.concatenate(kind), "k": np.concatenate(k_of), "delta": np.concatenate(delta_of),
            "other": np.concatenate(other), "singles": singles}


def records_from_positions(position, times=None, volume=1.0):
    """Impulse records with unit (or given) volumes: with row_code_table() an attenuated volume names its row."""
    position = np.asarray(position, np.float32).reshape(-1, 3)
    rec = aligned_zeros(position.shape[0], IMPULSE)
    rec["volume"] = np.float32(volume)
    rec["position"][:, :3] = position
    rec["time"] = (np.arange(position.shape[0]) + 100.25) / 44100.0 if times is None else times
    return rec


def boundary_set(frame):
    """The sweep of hrtf_boundary_records and, behind it, the named singles (sorted by name), as impulse records with unit volumes and
    time (i + 100.25) / 44100: (records, the builder's dict, names of the singles)."""
    b = hrtf_boundary_records(frame["facing"], frame["up"], frame["mic"], frame["radius"])
    names = sorted(b["singles"])
    pos = np.concatenate([b["position"], np.stack([b["singles"][n] for n in names])])
    return records_from_positions(pos), b, names


def describe(b, names, i):
    """What record i of boundary_set is: for failure messages."""
    n = b["position"].shape[0]
    if i >= n:
        return "single %s" % names[i - n]
    return "%s boundary k=%d delta=%+.3g (other angle %g)" % (b["kind"][i], b["k"][i], b["delta"][i], b["other"][i])


def row_code_table():
    """[2][360][180][8]: table[ear][row][band] = +-(row * 8 + band + 1), exact in binary32 (< 2^24): with unit volumes an attenuated
    volume names the row it was read from; the zero padding row reads as 0."""
    code = (np.arange(HRTF_ROWS * 8, dtype=np.float64) + 1.0).reshape(360, 180, 8)
    return np.stack([code, -code]).astype(np.float32)


def rows_from_codes(volume):
    """Inverse of row_code_table for unit input volumes: the row a [n][8] attenuated volume was read from (360 * 180: padding)."""
    v = np.abs(np.asarray(volume, np.float64)[:, 0])
    return np.where(v == 0, HRTF_ROWS, (v - 1) / 8).astype(np.int64)


# (row * g) mod 64800 is a permutation (g is coprime to 64800 = 2^5 3^4 5^2) under which the neighbours of a row — row +- 1 (elevation)
# and row +- 180 (azimuth, and g = 137 mod 360) — move by at least 0.37 * 64800 places
SPREAD_MULTIPLIER = 24617


def spread_table():
    """The table for the fast mode's test: [2][360][180][8] in (0, 1], a fixed permutation of the row numbers, so that a record
    attenuated with a NEIGHBOURING row (a +- 1, e +- 1) lands far outside the fast mode's rounding bound."""
    perm = (np.arange(HRTF_ROWS, dtype=np.int64) * SPREAD_MULTIPLIER) % HRTF_ROWS
    base = (perm + 1.0) / HRTF_ROWS
    band = (8.0 - np.arange(8)) / 8.0
    left = base[:, None] * band[None, :]
    right = (1.0 - base + 1.0 / HRTF_ROWS)[:, None] * band[None, :]
    return np.stack([left, right]).reshape(2, 360, 180, 8).astype(np.float32)


def neighbour_rows(row):
    """The rows next to `row` in azimuth and elevation, as the flat table is laid out (rows 0 .. 64799; the wrap is the table's)."""
    row = np.asarray(row, np.int64)
    return np.stack([(row + d) % HRTF_ROWS for d in (1, -1, 180, -180)])


def _shell(rng, n, centre, lo=2.0, hi=12.0):
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return (np.asarray(centre, np.float64) + d * rng.uniform(lo, hi, (n, 1))).astype(np.float32)


def time_edge_records(sample_rate, mic=(0.0, 0.0, 0.0)):
    """Impulse records whose TIMES are the edges of round(time * sample_rate) and of the predelay; positions on a seeded shell of
    2 .. 12 m around `mic`, volumes of mixed sign and magnitude.  In this order (the tests also take prefixes):
      1. one record at the earliest time (1 ms: it becomes the predelay), one 1 ulp and one 2 ulp above it;
      2. runs of 1, 2, 3, 4, 5, 8 and 9 records in seven neighbouring bins (the edges of the folds' unroll by 4), interleaved;
      3. a crowd of 300 records in one bin, volumes of mixed sign and magnitude 1e-3, 1, 30: the summation order shows;
      4. for k = 1 .. 3000 the binary32 time nearest (k + 0.5) / sample_rate and its two binary32 neighbours.
    Times below 1 ms are dropped from part 4: an HRTF ear moves a time by up to 0.3 ms, and a negative attenuated time is undefined in
    the reference's flattenImpulses (a negative float converted to an unsigned index) and in the oracle alike.
    Returns (records, info): info['half_k'], info['half_t'] the kept k and their [3] times (below, nearest, above), and the slices
    'runs', 'crowd', 'half' of the record array."""
    sr = np.float32(sample_rate)
    rng = np.random.default_rng(20240)
    t0 = np.float32(1e-3)
    head = np.array([t0, np.nextafter(t0, np.float32(1)), np.nextafter(np.nextafter(t0, np.float32(1)), np.float32(1))], np.float32)
    first_bin = int(np.ceil(2e-3 * float(sr)))
    runs = []
    for j, length in enumerate((1, 2, 3, 4, 5, 8, 9)):
        runs.extend((first_bin + j + rng.uniform(-0.3, 0.3)) / float(sr) for _ in range(length))
    runs = np.asarray(runs, np.float64)[rng.permutation(len(runs))].astype(np.float32)
    crowd = ((first_bin + 12 + rng.uniform(-0.3, 0.3, 300)) / float(sr)).astype(np.float32)
    k = np.arange(1, 3001)
    nearest = ((k + 0.5) / float(sr)).astype(np.float32)
    half = np.stack([np.nextafter(nearest, np.float32(0)), nearest, np.nextafter(nearest, np.float32(1))], -1)
    keep = half[:, 0] > head[2]
    half_k, half = k[keep], half[keep]
    times = np.concatenate([head, runs, crowd, half.ravel()])
    assert times.min() == t0 and (times >= np.float32(1e-3)).all()
    rec = aligned_zeros(times.shape[0], IMPULSE)
    rec["time"] = times
    rec["position"][:, :3] = _shell(rng, times.shape[0], mic)
    rec["volume"] = (rng.uniform(-1, 1, (times.shape[0], 8)) * rng.choice([1e-3, 1.0, 30.0], (times.shape[0], 1))).astype(np.float32)
    n_head, n_runs = head.shape[0], runs.shape[0]
    info = {"half_k": half_k, "half_t": half, "runs": slice(n_head, n_head + n_runs), "crowd": slice(n_head + n_runs, n_head + n_runs + 300),
            "half": slice(n_head + n_runs + 300, times.shape[0]), "run_bins": first_bin + np.arange(7), "crowd_bin": first_bin + 12}
    return rec, info


# Speakers of the speaker-edge set: (direction, coefficient).  The first three share the axis a record lies exactly opposite of, with
# coefficients 0, 1 and 0.5 (gains 1, -1 and exactly 0); two directions are not of unit length.
EDGE_SPEAKERS = [
    ((0.0, 0.0, 1.0), 0.0), ((0.0, 0.0, 1.0), 1.0), ((0.0, 0.0, 1.0), 0.5),
    ((0.0, 0.0, 2.0), 0.5), ((3.0, 0.0, 4.0), 0.7), ((-1.0, 0.0, -1.0), 0.5),
    ((1.0, 0.0, -1.0), 0.5), ((0.3, -0.2, 0.9), 0.25), ((0.0, -5.0, 0.0), 1.0),
]


def speaker_edge_records(mic):
    """Impulse records for the speaker gain (1 - k) + k * dot(normalize(normalize(pos - mic)), normalize(speaker)), kernel.cpp:505-535:
    degenerate normalisations, exact cancellation, and volumes at the edges of any(volume != 0).  No NaN or Inf inputs.
    Returns (records, names): names[i] says what record i is ('' for the ordinary filler records)."""
    mic32 = np.asarray(mic, np.float32)
    up1 = np.nextafter(mic32, np.float32(np.inf))
    dn1 = np.nextafter(mic32, np.float32(-np.inf))
    pos, names = [mic32.copy()], ["at the microphone"]
    for axis in range(3):
        for nb, word in ((up1, "+"), (dn1, "-")):
            p = mic32.copy()
            p[axis] = nb[axis]
            pos.append(p), names.append("microphone %s1 ulp on axis %d" % (word, axis))
    # offsets whose squares underflow: length3 == 0 although the vector is not zero (absorbed by a non-zero microphone coordinate)
    for off in ((1e-25, 0, 0), (0, -1e-25, 0), (1e-25, -1e-25, 1e-25), (3e-23, 1e-30, -1e-24), (1e-45, 0, 0)):
        pos.append((mic32.astype(np.float64) + off).astype(np.float32)), names.append("offset %r: squares underflow" % (off,))
    # large coordinates: squares still finite, and squares that overflow (length3 = inf, the normal becomes 0)
    for c in ((1e18, 0, 0), (1e18, -1e18, 1e18), (0, 1.8e19, 0), (3e19, 0, 0), (3e19, 3e19, -3e19), (0, 0, -1e30), (2e19, 2e19, 0)):
        pos.append(np.asarray(c, np.float32)), names.append("coordinates %r" % (c,))
    # exactly opposite the speakers on +z (the differences are exact), and exactly in front
    for dz in (-2.0, -0.5, 4.0):
        pos.append((mic32.astype(np.float64) + (0, 0, dz)).astype(np.float32)), names.append("on the speaker axis, dz=%g" % dz)
    pos.append((mic32.astype(np.float64) + (0, 3.0, 0)).astype(np.float32)), names.append("opposite the -y speaker")
    n_edge = len(pos)
    rng = np.random.default_rng(77)
    filler = _shell(rng, 230, mic32)
    pos = np.concatenate([np.stack(pos), filler])
    names += [""] * filler.shape[0]
    n = pos.shape[0]
    rec = aligned_zeros(n, IMPULSE)
    rec["position"][:, :3] = pos
    rec["volume"] = (rng.uniform(-1, 1, (n, 8)) * rng.choice([1e-3, 1.0, 30.0], (n, 1))).astype(np.float32)
    # about four records per bin at 44.1 kHz, none before 1 ms
    rec["time"] = (rng.uniform(50.0, 50.0 + n / 4.0, n) / 44100.0).astype(np.float32)
    tiny = np.float32(1e-45)                                    # the smallest subnormal
    sub = np.array([1e-45, -3e-45, 1e-40, -1e-39, 5e-39, -1.1e-38, 7e-42, 1e-41], np.float32)
    assert (np.abs(sub) < np.finfo(np.float32).tiny).all() and (sub != 0).all()
    special = n_edge + np.arange(0, 40)
    rec["volume"][special[0:8]] = np.float32(-0.0)              # any(volume != 0) is false: silent
    names[special[0]:special[8]] = ["volume -0.0 in all bands"] * 8
    rec["volume"][special[8:16]] = np.float32(-0.0)
    for j, i in enumerate(special[8:16]):
        rec["volume"][i, j] = tiny if j % 2 else -tiny          # one subnormal band keeps the record alive
        names[i] = "volume -0.0 with band %d subnormal" % j
    rec["volume"][special[16:24]] = sub
    rec["volume"][special[20:24]] *= np.float32(-1)
    names[special[16]:special[24]] = ["all bands subnormal"] * 8
    # the edge positions once more, with subnormal volumes
    k = min(16, n_edge)
    rec["position"][special[24:24 + k], :3] = pos[:k]
    rec["volume"][special[24:24 + k]] = sub
    for j, i in enumerate(special[24:24 + k]):
        names[i] = names[j] + ", subnormal volume"
    # every eighth record all-zero (quirk Q2: attenuates to {0, 0}): inserted, so that no edge record is lost
    out = aligned_zeros(n + n // 7, IMPULSE)
    out_names = []
    src = 0
    for i in range(out.shape[0]):
        if i % 8 == 7:
            out[i] = rec[src - 1]
            out[i]["volume"] = 0
            out_names.append("all-zero volume")
        else:
            out[i] = rec[src]
            out_names.append(names[src])
            src += 1
    assert src == n
    rec, names = out, out_names
    assert np.isfinite(rec["position"]).all() and np.isfinite(rec["volume"]).all()
    return rec, names
