"""Tables for Context.set_source_table (rvb_set_source_table of include/rvb_capi.h): a loudspeaker balloon — gain per octave band over
azimuth and elevation — resampled on the host into the [360][180][8] cells that the row selection of the reference's kernel `hrtf`
addresses.  Plain numpy, no GPU.

The cells follow the reference's truncating rule (kernel.cpp:569-584), row = a * 180 + e with
    a = (long) (azimuth + 180) % 360      azimuth in [a - 180, a - 179): one degree each, centre a - 179.5
    e = 90 - (long) elevation             truncation goes toward zero, so the equator cell e == 90 spans (-1, 1) degrees, centre 0;
                                          e < 90 spans [90 - e, 91 - e), e > 90 spans (89 - e, 90 - e]; e == 0 is the pole itself
Azimuth is atan2(x, z) and elevation atan2(y, hypot(x, z)) in the source's frame: z = facing, y = cross(facing, x), x = normalize(cross(up, facing)).
There is no interpolation between rows on the device: whatever smoothness a balloon has goes into the table here."""
import numpy as np

AZIMUTHS, ELEVATIONS, BANDS = 360, 180, 8


def cell_centres():
    """(azimuth [360][180], elevation [360][180]) in degrees: the centre of every (a, e) cell under the truncating row rule."""
    a = np.arange(AZIMUTHS, dtype=np.float64)
    e = np.arange(ELEVATIONS, dtype=np.float64)
    el = np.where(e < 90, 90.5 - e, np.where(e > 90, 89.5 - e, 0.0))
    el[0] = 90.0                                    # only the pole itself selects e == 0
    return np.broadcast_to((a - 179.5)[:, None], (AZIMUTHS, ELEVATIONS)).copy(), np.broadcast_to(el[None, :], (AZIMUTHS, ELEVATIONS)).copy()


def table_from_function(fn):
    """[360][180][8] float32: fn(azimuth_deg, elevation_deg) -> eight band gains, sampled at the cell centres.  fn is tried on the whole
    [360][180] arrays first (result [360][180][8]) and called cell by cell where it does not take arrays."""
    az, el = cell_centres()
    try:
        out = np.asarray(fn(az, el), dtype=np.float64)
        if out.shape != (AZIMUTHS, ELEVATIONS, BANDS):
            raise ValueError(out.shape)
    except (TypeError, ValueError):
        out = np.array([[np.asarray(fn(float(az[i, j]), float(el[i, j])), dtype=np.float64).reshape(BANDS) for j in range(ELEVATIONS)]
                        for i in range(AZIMUTHS)])
    assert np.isfinite(out).all(), "a gain that is not finite"
    return out.astype(np.float32)


def polar_pattern(shape):
    """fn for table_from_function: the first-order pattern (1 - shape_b) + shape_b * cos(angle to the facing), the expression of
    rvb_set_source_pattern in the source's own frame; shape a scalar or eight values."""
    s = np.broadcast_to(np.asarray(shape, dtype=np.float64).reshape(-1), (BANDS,))

    def fn(az, el):
        d = np.cos(np.radians(az)) * np.cos(np.radians(el))
        return (1.0 - s) + s * np.asarray(d)[..., None]
    return fn


def table_from_balloon(az_deg, el_deg, gains):
    """[360][180][8] float32 from a regular balloon grid: gains [na][ne][8] (or [na][ne]: the same in every band) measured at the
    azimuths az_deg [na] and elevations el_deg [ne], both ascending, in degrees in the source's frame.  Bilinear in (azimuth, elevation)
    at the cell centres; the azimuth wraps round (a grid that lists both -180 and 180 may: the last column is then dropped), the elevation
    is held beyond the grid's first and last ring."""
    az = np.asarray(az_deg, dtype=np.float64).reshape(-1)
    el = np.asarray(el_deg, dtype=np.float64).reshape(-1)
    g = np.asarray(gains, dtype=np.float64)
    if g.ndim == 2:
        g = np.repeat(g[:, :, None], BANDS, axis=2)
    assert g.shape == (az.shape[0], el.shape[0], BANDS), "gains: [na][ne][8]"
    assert az.shape[0] >= 1 and el.shape[0] >= 1 and (np.diff(az) > 0).all() and (np.diff(el) > 0).all(), "ascending grids"
    assert az[-1] - az[0] <= 360.0, "azimuths span more than one turn"
    if az.shape[0] > 1 and az[-1] - az[0] == 360.0:
        az, g = az[:-1], g[:-1]
    # one period before and behind, so that every centre has a neighbour on both sides
    az_ext = np.concatenate([az - 360.0, az, az + 360.0])
    g_ext = np.concatenate([g, g, g], axis=0)
    caz, cel = cell_centres()
    caz, cel = caz[:, 0], cel[0, :]
    caz = az[0] + np.mod(caz - az[0], 360.0)                       # into [az[0], az[0] + 360)
    hi = np.clip(np.searchsorted(az_ext, caz, side="right"), 1, az_ext.shape[0] - 1)
    lo = hi - 1
    wa = (caz - az_ext[lo]) / (az_ext[hi] - az_ext[lo])
    rows = g_ext[lo] * (1.0 - wa)[:, None, None] + g_ext[hi] * wa[:, None, None]         # [360][ne][8]
    if el.shape[0] == 1:
        out = np.repeat(rows, ELEVATIONS, axis=1)
    else:
        c = np.clip(cel, el[0], el[-1])
        ehi = np.clip(np.searchsorted(el, c, side="right"), 1, el.shape[0] - 1)
        elo = ehi - 1
        we = (c - el[elo]) / (el[ehi] - el[elo])
        out = rows[:, elo] * (1.0 - we)[None, :, None] + rows[:, ehi] * we[None, :, None]
    assert np.isfinite(out).all(), "a gain that is not finite"
    return out.astype(np.float32)


def normalised(v):
    """A facing or up vector of any non-zero length as the unit vector rvb_set_source_table expects: binary64 in, binary32 out."""
    v = np.asarray(v, dtype=np.float64)
    n = np.linalg.norm(v, axis=-1, keepdims=True)
    assert (n > 0).all() and np.isfinite(n).all(), "a vector of zero length"
    return (v / n).astype(np.float32)


def balloon_gradient(grad, rows):
    """The float64 [360][180][8] sums by table row of per-ray or per-image gain derivatives: grad [n][8] (dL/dg of capi.Context.source_grad
    or source_grad_images) and rows [n] (their table rows) as numpy arrays or torch tensors.  Entry [a][e][b] is dL/dtable[a][e][b] of the
    source table that the records reflect; a row of 64800 or above — the zero row behind the table — belongs to no cell and adds nothing.
    Added in binary64 in the order of the rays (images)."""
    if hasattr(grad, "cpu"):
        grad = grad.cpu().numpy()
    if hasattr(rows, "cpu"):
        rows = rows.cpu().numpy()
    grad = np.asarray(grad, dtype=np.float64).reshape(-1, 8)
    rows = np.asarray(rows).reshape(-1).astype(np.int64) & 0xFFFFFFFF      # (an int32 tensor holds the unsigned row)
    assert grad.shape[0] == rows.shape[0], "balloon_gradient: a row per gradient entry"
    out = np.zeros((360 * 180, 8), dtype=np.float64)
    inside = rows < 360 * 180
    np.add.at(out, rows[inside], grad[inside])
    return out.reshape(360, 180, 8)

