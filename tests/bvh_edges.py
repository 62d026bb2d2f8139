"""Builders of constructed scenes for the trace stage: the BVH builder (csrc/bvh_build.hip), the three path kernels, the image check and
the shadow kernels.  A plain module: no fixtures, no GPU, no oracle — tests/test_bvh_edge_inputs.py checks with the CPU oracle that
these inputs hold what they are built for, tests/test_bvh_host.py runs the builder alone over them, tests/test_gpu_bvh_edges.py feeds
them to the kernels.

Every builder returns (scene, mic, source, directions, nreflections), a pure function of its arguments (fixed seeds).  `source` is one
point, or [m][3] points where a set asks for many traces of one scene with the same rays (sources_of() gives [m][3] either way; the GPU
tests put such a set into a few several-pairs launches).  Surfaces are assigned as triangle index % 5 over five surfaces of distinct
random coefficients, so that WHICH of several tied triangles won a hit shows in the volumes."""
import numpy as np

from parallel_reverb_raytracer_amd import scenes
from parallel_reverb_raytracer_amd.dtypes import SURFACE, TRIANGLE, aligned_zeros, float3_array

NSURFACES = 5
TINY_SEEDS = {1: 0, 2: 0, 3: 0, 4: 0, 5: 0, 8: 0, 9: 0}        # per k: the first seed with >= 20 rays that hit and >= 20 that escape (oracle)
AXES = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], np.float64)
BOX_MIC = (3.3, 2.2, 4.6)
BOX_SOURCE = (2.0, 1.5, 3.0)                                 # above a floor vertex: the axis rays meet vertices
FAR_OFFSETS = (1e3, 7e4, 1e6)
FAR_SCALED = (5e8, 512.0)                                    # offset and scale of the fourth `far` scene


def surfaces():
    rng = np.random.default_rng(5)
    s = aligned_zeros(NSURFACES, SURFACE)
    s["specular"] = rng.uniform(0.5, 0.99, (NSURFACES, 8)).astype(np.float32)
    s["diffuse"] = rng.uniform(0.3, 0.95, (NSURFACES, 8)).astype(np.float32)
    return s


def make_scene(verts, tris):
    """verts [nv][3], tris [nt][3] vertex indices -> (TRIANGLE records with surface = index % 5, [nv][4] float32, the five surfaces)."""
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    t = aligned_zeros(tris.shape[0], TRIANGLE)
    t["surface"] = np.arange(tris.shape[0]) % NSURFACES
    t["v0"], t["v1"], t["v2"] = tris[:, 0], tris[:, 1], tris[:, 2]
    return t, float3_array(np.asarray(verts, np.float64).reshape(-1, 3)), surfaces()


def soup_scene(corners):
    """corners [nt][3][3]: every triangle gets three vertices of its own."""
    corners = np.asarray(corners, np.float64).reshape(-1, 3, 3)
    return make_scene(corners.reshape(-1, 3), np.arange(corners.shape[0] * 3).reshape(-1, 3))


def reversed_order(scene):
    """The same triangles in reverse order (surfaces again index % 5): equal geometry, every tie has another lowest index."""
    t, v, s = scene
    r = aligned_zeros(t.shape[0], TRIANGLE)
    r["v0"], r["v1"], r["v2"] = t["v0"][::-1], t["v1"][::-1], t["v2"][::-1]
    r["surface"] = np.arange(t.shape[0]) % NSURFACES
    return r, v, s


def sources_of(case):
    return np.asarray(case[2], np.float64).reshape(-1, 3)


def unit(d):
    d = np.asarray(d, np.float64).reshape(-1, 3)
    return float3_array(d / np.linalg.norm(d, axis=1, keepdims=True))


def axis_and_sphere(nsphere, seed):
    """The six axis directions (exact), then `nsphere` seeded sphere directions."""
    return float3_array(np.concatenate([AXES, scenes.sphere_directions(nsphere, seed=seed)[:, :3].astype(np.float64)]))


# ---- tiny trees: a root with 1 - 3 children, leaves of 1, 2 and 3 triangles, no triangle at all ----------------------------------

def tiny(k):
    """k seeded random triangles of 1 - 3 m around the origin (an open scene), 257 rays x 5 reflections."""
    rng = np.random.default_rng(1000 * k + TINY_SEEDS[k])
    centre = rng.uniform(-1.0, 1.0, (k, 1, 3))
    size = rng.uniform(1.0, 3.0, (k, 1, 1))
    corners = centre + rng.uniform(-0.5, 0.5, (k, 3, 3)) * size
    return soup_scene(corners), (0.4, -0.3, 0.2), (0.1, 0.2, -0.1), scenes.sphere_directions(257, seed=11), 5


def tetrahedron():
    """A closed tetrahedron (4 triangles: one full leaf) with source and microphone inside."""
    v = [(2, 2, 2), (2, -2, -2), (-2, 2, -2), (-2, -2, 2)]
    return make_scene(v, [(0, 1, 2), (0, 3, 1), (0, 2, 3), (1, 3, 2)]), (-0.3, 0.2, 0.25), (0.2, 0.1, -0.1), scenes.sphere_directions(257, seed=12), 5


def none_hittable():
    """Six zero-area triangles and one with a NaN vertex: the builder drops all seven (the root of inverted boxes, stack_need 0)."""
    rng = np.random.default_rng(7)
    corners = []
    for i in range(6):
        a, b = rng.uniform(-2, 2, 3), rng.uniform(-2, 2, 3)
        corners.append([a, a, b] if i % 2 else [a, b, a + 0.5 * (b - a)])       # a repeated corner / three corners on one line
    corners.append([(0.0, 0.0, 1.0), (1.0, 0.0, 1.0), (np.nan, 1.0, 1.0)])
    return soup_scene(corners), (0.4, -0.3, 0.2), (0.1, 0.2, -0.1), scenes.sphere_directions(257, seed=13), 5


# ---- the tessellated box: exact ties across leaves and subtrees --------------------------------------------------------------------

def _face(origin, du, dv, n):
    """(n + 1)^2 vertices origin + i du + j dv and 2 n^2 triangles: cell (i, j) is (a, b, c), (a, c, d) with a = (i, j), b = (i + 1, j),
    c = (i + 1, j + 1), d = (i, j + 1), so six triangles meet at every interior vertex."""
    i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    verts = np.asarray(origin, np.float64) + i[..., None] * np.asarray(du, np.float64) + j[..., None] * np.asarray(dv, np.float64)
    idx = np.arange((n + 1) ** 2).reshape(n + 1, n + 1)
    a, b, c, d = idx[:-1, :-1], idx[1:, :-1], idx[1:, 1:], idx[:-1, 1:]
    tris = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)])
    return verts.reshape(-1, 3), tris


def grid_box_scene(n=8, offset=0.0, scale=1.0, extra_vertices=()):
    """An axis-aligned 8 x 4 x 8 m box, every face n x n cells of two triangles: floor (y = 0) first, then the ceiling, then the four
    walls; 12 n^2 triangles.  For n = 8 the vertices are multiples of 0.5 m.  Every coordinate is scaled, then offset."""
    w, h, d = 8.0, 4.0, 8.0
    faces = [((0, 0, 0), (w / n, 0, 0), (0, 0, d / n)), ((0, h, 0), (w / n, 0, 0), (0, 0, d / n)),
             ((0, 0, 0), (w / n, 0, 0), (0, h / n, 0)), ((0, 0, d), (w / n, 0, 0), (0, h / n, 0)),
             ((0, 0, 0), (0, 0, d / n), (0, h / n, 0)), ((w, 0, 0), (0, 0, d / n), (0, h / n, 0))]
    verts, tris, base = [], [], 0
    for origin, du, dv in faces:
        v, t = _face(origin, du, dv, n)
        verts.append(v), tris.append(t + base)
        base += v.shape[0]
    verts = np.concatenate(verts) * scale + offset
    if len(extra_vertices):
        verts = np.concatenate([verts, np.asarray(extra_vertices, np.float64).reshape(-1, 3)])
    return make_scene(verts, np.concatenate(tris))


def interior_floor_vertices(n=8):
    return [(i, j) for i in range(1, n) for j in range(1, n)]


def grid_box_vertex_rays(n=8):
    """One trace per interior floor vertex (i, j), the source at (i, 1.5, j): the up and the down ray bounce between a floor vertex and a
    ceiling vertex, a six-way tie at every bounce, starting on the tied triangles each time.  64 rays x 6 reflections per source."""
    src = [(float(i), 1.5, float(j)) for i, j in interior_floor_vertices(n)]
    return grid_box_scene(n), BOX_MIC, np.asarray(src), axis_and_sphere(58, seed=14), 6


def grid_box_edge_rays(n=8):
    """Sources above the middles of the floor's cell edges, (i + 0.5, 1.5, j) and (i, 1.5, j + 0.5): the vertical rays meet an edge
    that two triangles share.  The same 64 rays x 6 reflections."""
    src = [(i + 0.5, 1.5, float(j)) for i in range(n) for j in range(1, n)] + [(float(i), 1.5, j + 0.5) for i in range(1, n) for j in range(n)]
    return grid_box_scene(n), BOX_MIC, np.asarray(src), axis_and_sphere(58, seed=14), 6


def grid_box_junction_rays(n=8):
    """Diagonal rays from (2, 1.5, 3) towards the points (x, 0, 0) and (0, 0, z) of the two wall-floor junction lines, x and z in steps
    of 0.5 m: the tied triangles there have DIFFERENT normals (floor and wall)."""
    src = np.array([2.0, 1.5, 3.0])
    steps = np.arange(0.0, 8.25, 0.5)
    targets = [(x, 0.0, 0.0) for x in steps] + [(0.0, 0.0, z) for z in steps]
    return grid_box_scene(n), BOX_MIC, tuple(src), unit(np.asarray(targets) - src), 6


def stray_vertex():
    """The box plus one vertex at (1e7, 0, 0) that no triangle refers to: the builder's coordinate range counts it (pad = 200 m, every
    box is entered, no own-plane skip), the oracle never reads it."""
    return grid_box_scene(8, extra_vertices=[(1e7, 0.0, 0.0)]), BOX_MIC, BOX_SOURCE, axis_and_sphere(250, seed=3), 8


def far(which):
    """which = 0, 1, 2: the box translated by (t, t, t), t = FAR_OFFSETS[which]; which = 3: the box scaled by 512 at t = 5e8.  Source and
    microphone are scaled and translated with it; 6 axis + 250 sphere directions, 8 reflections.  Every vertex and the source stay exact
    in binary32 (multiples of 0.5 m at t <= 1e6 where an ulp is 1/16 m, multiples of 256 m at 5e8 where it is 32 m)."""
    t, s = (FAR_OFFSETS[which], 1.0) if which < 3 else FAR_SCALED
    move = lambda p: tuple(np.asarray(p, np.float64) * s + t)
    return grid_box_scene(8, offset=t, scale=s), move(BOX_MIC), move(BOX_SOURCE), axis_and_sphere(250, seed=3), 8


BLOCKED_MIC = (6.0, 1.5, 3.0)                                # on the x axis ray of BOX_SOURCE


def far_blocked(occluder=True):
    """The scaled box at 5e8 with the microphone at (6, 1.5, 3) (box coordinates) and a 1 x 1 m panel at x = 4 between it and the source:
    the direct path and the shadow ray of the -x axis ray's first hit, (0, 1.5, 3) -> microphone, run along (1, 0, 0) EXACTLY and are
    blocked by the panel.  Two direction components are zero and the origin's coordinates are above 3.4e8, where the product of a
    coordinate and an inverse direction clamped too high (clamp_inv, csrc/traversal.h) is no longer finite.  occluder=False: the same without the panel."""
    t, s = FAR_SCALED
    tris, verts, surf = grid_box_scene(8, offset=t, scale=s)
    if occluder:
        panel = np.array([(4, 1, 2.5), (4, 2, 2.5), (4, 2, 3.5), (4, 1, 3.5)], np.float64) * s + t
        base = verts.shape[0]
        verts = np.concatenate([verts[:, :3].astype(np.float64), panel])
        corner = np.stack([tris["v0"], tris["v1"], tris["v2"]], -1).astype(np.int64)
        tris, verts, surf = make_scene(verts, np.concatenate([corner, [(base, base + 1, base + 2), (base, base + 2, base + 3)]]))
    move = lambda p: tuple(np.asarray(p, np.float64) * s + t)
    return (tris, verts, surf), move(BLOCKED_MIC), move(BOX_SOURCE), axis_and_sphere(250, seed=3), 8


# ---- more than four exact duplicates; thin parallel sheets -------------------------------------------------------------------------

DUPLICATES = 300


def duplicates():
    """One 2 m triangle 300 times (300 copies of its vertices): 75 leaves of equal boxes, the lowest index must win.  300 rays x 4."""
    one = np.array([(0.0, 0.0, 0.0), (2.0, 0.0, 0.0), (0.0, 2.0, 0.0)])
    return soup_scene(np.repeat(one[None], DUPLICATES, 0)), (0.5, 0.4, 0.7), (0.5, 0.5, 0.4), scenes.sphere_directions(300, seed=16), 4


def duplicate_tetrahedron():
    """A closed tetrahedron whose four faces are 300-fold each, interleaved: triangle 4 c + f is copy c of face f (1 200 triangles)."""
    v = np.array([(2, 2, 2), (2, -2, -2), (-2, 2, -2), (-2, -2, 2)], np.float64)
    faces = np.array([(0, 1, 2), (0, 3, 1), (0, 2, 3), (1, 3, 2)])
    corners = np.tile(v[faces], (DUPLICATES, 1, 1))                      # [300 * 4][3][3]: face = index % 4
    return soup_scene(corners), (-0.3, 0.2, 0.25), (0.2, 0.1, -0.1), scenes.sphere_directions(300, seed=17), 4


def _sheet_directions():
    """Along the stack normal (+-z) and at 1 .. 5 degrees to it, ten azimuths each."""
    out = [(0.0, 0.0, 1.0), (0.0, 0.0, -1.0)]
    for deg in (1, 2, 3, 4, 5):
        for a in np.arange(10) * (2 * np.pi / 10) + 0.1:
            for sign in (1.0, -1.0):
                out.append((np.sin(np.radians(deg)) * np.cos(a), np.sin(np.radians(deg)) * np.sin(a), sign * np.cos(np.radians(deg))))
    return unit(out)


def stacked_sheets(inside=False):
    """300 parallel 1 m triangles 1 mm apart (z = k mm); the source in front of the stack, or between sheets 150 and 151."""
    k = np.arange(300, dtype=np.float64) * 1e-3
    corners = np.stack([np.stack([0 * k, 0 * k, k], -1), np.stack([0 * k + 1, 0 * k, k], -1), np.stack([0 * k, 0 * k + 1, k], -1)], 1)
    source = (0.25, 0.25, 0.1505) if inside else (0.25, 0.25, -0.5)
    return soup_scene(corners), (0.3, 0.2, -0.8), source, _sheet_directions(), 4


# ---- a deep traversal stack ----------------------------------------------------------------------------------------------------------

def peel(mirrored=False):
    """Triangles whose sizes and distances from the origin grow geometrically over eleven decades: the SAH builder peels them off one
    small group at a time, depth 15 and stack_need 45 of the 64 entries.  For k = 0 .. 229 (x_k = 1e-3 * 1.12^k <= 2e8) and j = 0, 1, 2
    one triangle (x_k, 3 j z, 0), (x_k + z, 3 j z, 0), (x_k, 3 j z + z, 0.1 z) with z = max(0.05, 2e-3 x_k): 690 triangles.  The box
    padding is 3.7 km, so near the origin every box contains every ray origin.  One ray per triangle, towards its centroid.
    mirrored: x -> -x and the triangle order reversed, which puts the deep chain into other child slots."""
    corners = []
    k = 0
    while 1e-3 * 1.12 ** k <= 2e8:
        x = 1e-3 * 1.12 ** k
        z = max(0.05, 2e-3 * x)
        for j in range(3):
            corners.append([(x, 3 * j * z, 0.0), (x + z, 3 * j * z, 0.0), (x, 3 * j * z + z, 0.1 * z)])
        k += 1
    corners = np.asarray(corners, np.float64)
    source, mic = np.array([0.0, 0.0, 50.0]), np.array([0.5, 0.5, 20.0])
    if mirrored:
        corners = corners[::-1].copy()
        corners[:, :, 0] *= -1.0
        mic[0] *= -1.0
    centroids = corners.astype(np.float32).astype(np.float64).mean(axis=1)
    return soup_scene(corners), tuple(mic), tuple(source), unit(centroids - source), 4


def all_cases():
    """name -> builder of every case (built on demand: the tests share the built cases through a module fixture)."""
    c = {"tiny_%d" % k: (lambda k=k: tiny(k)) for k in sorted(TINY_SEEDS)}
    c.update({"tetrahedron": tetrahedron, "none_hittable": none_hittable,
              "grid_box_vertex_rays": grid_box_vertex_rays, "grid_box_edge_rays": grid_box_edge_rays, "grid_box_junction_rays": grid_box_junction_rays,
              "duplicates": duplicates, "duplicate_tetrahedron": duplicate_tetrahedron,
              "stacked_sheets": stacked_sheets, "stacked_sheets_inside": lambda: stacked_sheets(True),
              "peel": peel, "peel_mirrored": lambda: peel(True), "stray_vertex": stray_vertex})
    c.update({"far_%d" % w: (lambda w=w: far(w)) for w in range(4)})
    c["far_3_blocked"] = far_blocked
    return c
