"""Builders of one small non-convex room for the image-source stage (image_plan_kernel / image_check_kernel, csrc/image_kernels.hip) and
every pass that rewrites its results: reshade_images_kernel, the image stage of rvb_relisten, source_pattern_images_kernel and
source_table_images_kernel.  A plain module: no fixtures, no GPU, no oracle — tests/test_image_edge_inputs.py checks with the CPU oracle
that these inputs hold what they are built for (image sources of every order 1 .. 9 in every pair, items that a closest-hit or visibility
query rejects, a hidden direct path, escaping rays, chains that die in one band), tests/test_gpu_image_edges.py feeds them to the kernels.

Every builder is a pure function of its arguments (fixed seeds)."""
import numpy as np

from parallel_reverb_raytracer_amd import scenes
from parallel_reverb_raytracer_amd.dtypes import AIR_COEFFICIENTS, SURFACE, TRIANGLE, aligned_zeros, float3_array

from bvh_edges import grid_box_scene
from test_gpu_reshade import AIR_B, set_b

NSURFACES = 14                                               # one per triangle: 12 of the box, 2 of the panel
PANEL = ((4.0, 0.5, 2.5), (4.0, 3.0, 2.5), (4.0, 3.0, 5.0), (4.0, 0.5, 5.0))     # x = 4, y in [0.5, 3], z in [2.5, 5]
# (microphone, source): both on one side of the panel and in view of each other; twice the panel between them
PAIRS = (((3.3, 2.2, 4.6), (2.0, 1.5, 3.0)), ((6.5, 1.0, 6.0), (1.5, 2.5, 1.0)), ((5.5, 3.0, 3.5), (2.5, 1.0, 4.0)))
MICS = np.array([p[0] for p in PAIRS], np.float32)
SOURCES = np.array([p[1] for p in PAIRS], np.float32)
DIRECT_VISIBLE = (True, False, False)
MAIN = (509, 12)
# 130 x 32: nreflections % 32 == 0, the 16-bit key runs; 64 x 1, 2, 8, 9, 10: around min(nreflections, 9) and around the first order that
# reads the ray's record index - 1; 5 x 12: fewer rays than a wave
EDGE_SHAPES = ((130, 32), (64, 1), (64, 2), (64, 8), (64, 9), (64, 10), (5, 12))
DEAD_BAND = 3                                                # set_b: the band in which DEAD_SURFACE reflects nothing specularly under table B
DEAD_SURFACE, DEAD_DIFFUSE, MUTE = 0, 4, 7                   # a floor triangle; band 5 of a wall; a wall without any diffuse reflection
RAY_OFFSET = 2 ** 32 + 5


def surfaces():
    """14 surfaces of distinct seeded coefficients per band: which triangles a chain went over, and how many, shows in every band."""
    rng = np.random.default_rng(21)
    s = aligned_zeros(NSURFACES, SURFACE)
    s["specular"] = rng.uniform(0.6, 0.99, (NSURFACES, 8)).astype(np.float32)
    s["diffuse"] = rng.uniform(0.3, 0.95, (NSURFACES, 8)).astype(np.float32)
    return s


def room(panel=True, hole=False):
    """An 8 x 4 x 8 m box of two triangles per wall (bvh_edges.grid_box_scene(1): floor, ceiling, the walls z = 0, z = 8, x = 0, x = 8),
    then the free-standing panel, last in the list: the wall triangles have the same numbers with and without it.  hole: without the last
    wall triangle (half of the wall x = 8), so that rays escape.  Triangle t has surface t of the 14 in every variant (with the hole the
    panel's triangles are 11 and 12 and keep the surfaces 12 and 13)."""
    box, verts, _ = grid_box_scene(1)
    corner = np.stack([box["v0"], box["v1"], box["v2"]], -1).astype(np.int64)
    surface = np.arange(12)
    verts = verts[:, :3].astype(np.float64)
    if hole:
        corner, surface = corner[:-1], surface[:-1]
    if panel:
        base = verts.shape[0]
        verts = np.concatenate([verts, np.asarray(PANEL, np.float64)])
        corner = np.concatenate([corner, [(base, base + 1, base + 2), (base, base + 2, base + 3)]])
        surface = np.concatenate([surface, [12, 13]])
    t = aligned_zeros(corner.shape[0], TRIANGLE)
    t["surface"] = surface
    t["v0"], t["v1"], t["v2"] = corner[:, 0], corner[:, 1], corner[:, 2]
    return t, float3_array(verts), surfaces()


def table_b():
    """The other surface table, as tests/test_gpu_reshade.py makes its own: every coefficient changed, band 3 of a floor triangle without
    specular reflection (the chains over it die in that band: the sign of the zero is compared), one wall without diffuse reflection."""
    return set_b(surfaces(), DEAD_SURFACE, DEAD_DIFFUSE, MUTE)


def with_table(scene, table):
    return scene[0], scene[1], table


def directions(nrays):
    return scenes.sphere_directions(nrays, seed=11)


def tables():
    """name -> (surface table, air): A the room's own, B the other"""
    return {"A": (surfaces(), AIR_COEFFICIENTS), "B": (table_b(), AIR_B)}
