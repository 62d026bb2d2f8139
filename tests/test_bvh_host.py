"""The BVH builder alone (csrc/bvh_build.hip, host code): tests/cpp/bvh_dump.cpp is compiled together with it into a temporary directory
and run over every scene of tests/bvh_edges.py and three seeded ones; what it wrote is checked here in numpy, independently of the
builder's code — partition, box containment after the binary16 outward rounding, tree shape, the worst-case stack, the own-plane skip,
and what the builder refuses.  No GPU, nothing loaded into Python."""
import os
import subprocess

import numpy as np
import pytest

import bvh_edges as E
from parallel_reverb_raytracer_amd import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "parallel-reverb-raytracer_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

EMPTY, LEAF, NODE_SHIFT, MAX_LEAF, STACK = 0xFFFFFFFF, 0x80000000, 6, 4, 64       # csrc/bvh.h
EPSILON = 1e-4                                                                       # RVB_EPSILON
CHILD = np.dtype([("lox", "<u2"), ("hix", "<u2"), ("loy", "<u2"), ("hiy", "<u2"), ("loz", "<u2"), ("hiz", "<u2"), ("ref", "<u4")])
BVH_TRI = np.dtype([("v0", "<f4", (3,)), ("e0", "<f4", (3,)), ("e1", "<f4", (3,)), ("index", "<u4"), ("surface", "<u4"), ("pad", "<u4")])
TRI_SHADE = np.dtype([("n", "<f4", (3,)), ("surface", "<u4"), ("skip_ref", "<u4"), ("skip_a", "<f4"), ("skip_b", "<f4"), ("group", "<u4")])
assert CHILD.itemsize == 16 and BVH_TRI.itemsize == 48 and TRI_SHADE.itemsize == 32


def build_dump_tool(directory):
    """Compiles csrc/bvh_build.hip and tests/cpp/bvh_dump.cpp as host code and links them; returns the program's path."""
    directory = str(directory)
    tool = os.path.join(directory, "bvh_dump")
    if os.path.exists(tool):
        return tool
    objects = []
    for src in (os.path.join(CSRC, "bvh_build.hip"), os.path.join(ROOT, "tests", "cpp", "bvh_dump.cpp")):
        obj = os.path.join(directory, os.path.basename(src) + ".o")
        subprocess.check_call([HIPCC, "--cuda-host-only", "-x", "hip", "-std=c++17", "-O1", "-ffp-contract=off", "-I" + CSRC, "-c", src, "-o", obj])
        objects.append(obj)
    subprocess.check_call([HIPCC, "-o", tool] + objects)
    return tool


def run_dump(tool, scene, directory):
    """The builder's output for a scene: dict with nodes [n][4] CHILD, tris, shade, leafpos, depth, stack_need, pad, error."""
    directory = str(directory)
    os.makedirs(directory, exist_ok=True)
    triangles, vertices, surfaces = scene
    np.ascontiguousarray(triangles).tofile(os.path.join(directory, "triangles.bin"))
    np.ascontiguousarray(vertices, dtype=np.float32).tofile(os.path.join(directory, "vertices.bin"))
    subprocess.run([tool, os.path.join(directory, "triangles.bin"), os.path.join(directory, "vertices.bin"), str(surfaces.shape[0]), directory],
                   check=True, timeout=120)
    depth, stack_need, pad_bits = open(os.path.join(directory, "meta.txt")).read().split()
    load = lambda name, dtype: np.fromfile(os.path.join(directory, name), dtype=dtype)
    return {"nodes": load("nodes.bin", CHILD).reshape(-1, 4), "tris": load("tris.bin", BVH_TRI), "shade": load("shade.bin", TRI_SHADE),
            "leafpos": load("leafpos.bin", np.uint32), "depth": int(depth), "stack_need": int(stack_need),
            "pad": np.array([int(pad_bits)], np.uint32).view(np.float32)[0], "error": open(os.path.join(directory, "error.txt")).read()}


def host_scenes():
    """name -> scene: one entry per distinct scene of bvh_edges.py, and three of the seeded scenes of the parity tests."""
    from test_gpu_parity import triangle_soup
    out = {}
    for name, make in E.all_cases().items():
        if name.startswith("grid_box_") and "grid_box" in out:
            continue
        out["grid_box" if name.startswith("grid_box_") else name] = make()[0]
    out["room_768"] = scenes.rotated_square_room(8)
    out["cathedral_3k"] = scenes.cathedral(3000)[0]
    out["soup_1"] = triangle_soup(1)
    return out


SCENE_NAMES = sorted({"grid_box" if n.startswith("grid_box_") else n for n in E.all_cases()} | {"room_768", "cathedral_3k", "soup_1"})
ROOMS_WITH_SKIPS = ("grid_box", "room_768")


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    return build_dump_tool(tmp_path_factory.mktemp("bvh_dump"))


@pytest.fixture(scope="module")
def built(tool, tmp_path_factory):
    base = tmp_path_factory.mktemp("bvh_scenes")
    out = {}
    for name, scene in host_scenes().items():
        dump = run_dump(tool, scene, base / name)
        assert dump["error"] == "", name
        out[name] = (scene, Tree(scene, dump))
    return out


def corners_of(scene):
    """[nt][3][3] binary32 corners by original triangle index."""
    t, v, _ = scene
    v = np.asarray(v, np.float32)[:, :3]
    return np.stack([v[t["v0"]], v[t["v1"]], v[t["v2"]]], 1)


def expected_pad(scene):
    v = np.asarray(scene[1], np.float32)[:, :3]
    finite = np.abs(v[np.isfinite(v)])
    maxabs = finite.max() if finite.size else np.float32(0)
    return max(np.float32(1e-3), np.float32(2e-5) * np.float32(maxabs))


def half_planes(bits):
    return np.ascontiguousarray(bits).view(np.float16).astype(np.float32)


class Tree:
    """The dumped tree with what the checks need: decoded planes, the leaf positions under every child reference."""

    def __init__(self, scene, dump):
        self.scene, self.dump = scene, dump
        self.nodes, self.tris, self.shade, self.leafpos = dump["nodes"], dump["tris"], dump["shade"], dump["leafpos"]
        self.ref = self.nodes["ref"]
        self.lo = np.stack([half_planes(self.nodes[a]) for a in ("lox", "loy", "loz")], -1)          # [n][4][3]
        self.hi = np.stack([half_planes(self.nodes[a]) for a in ("hix", "hiy", "hiz")], -1)
        self.corners = corners_of(scene)
        self._under = {}

    @staticmethod
    def leaf_range(ref):
        return int(ref & 0x0FFFFFFF), int((ref >> 28) & 7) + 1

    def children(self, node):
        return [int(r) for r in self.ref[node] if r != EMPTY]

    def under(self, ref):
        """Leaf positions of every triangle below a child reference."""
        ref = int(ref)
        if ref not in self._under:
            if ref & LEAF:
                first, count = self.leaf_range(ref)
                self._under[ref] = np.arange(first, first + count)
            else:
                parts = [self.under(c) for c in self.children(ref >> NODE_SHIFT)]
                self._under[ref] = np.concatenate(parts) if parts else np.zeros(0, np.int64)
        return self._under[ref]

    def leaves(self):
        return [self.leaf_range(r) for r in self.ref.reshape(-1) if r != EMPTY and r & LEAF]


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_partition(built, name):
    scene, tree = built[name]
    ntri = scene[0].shape[0]
    corners = tree.corners.astype(np.float64)
    e0, e1 = corners[:, 1] - corners[:, 0], corners[:, 2] - corners[:, 0]
    with np.errstate(invalid="ignore"):
        dropped = ~np.isfinite(corners).all(axis=(1, 2)) | (np.linalg.norm(np.cross(e0, e1), axis=1) * 2.02 < EPSILON)
    kept = np.nonzero(~dropped)[0]
    assert tree.shade.shape[0] == tree.leafpos.shape[0] == ntri
    # every kept triangle in exactly one leaf, every dropped one in none; leafpos is the inverse map
    assert np.array_equal(np.sort(tree.tris["index"]), kept)
    assert (tree.leafpos[dropped] == 0xFFFFFFFF).all()
    assert np.array_equal(tree.leafpos[tree.tris["index"]], np.arange(tree.tris.shape[0]))
    # the leaves tile the leaf-order array, hold 1 - 4 triangles each, in ascending original index
    leaves = sorted(tree.leaves())
    position = 0
    for first, count in leaves:
        assert first == position and 1 <= count <= MAX_LEAF
        assert (np.diff(tree.tris["index"][first:first + count].astype(np.int64)) > 0).all()
        position += count
    assert position == tree.tris.shape[0]
    # stored v0, e0, e1: the binary32 corner and the binary32 differences of the corners (bit for bit)
    c32 = tree.corners[tree.tris["index"]]
    assert c32[:, 0].tobytes() == tree.tris["v0"].tobytes()
    assert (c32[:, 1] - c32[:, 0]).tobytes() == tree.tris["e0"].tobytes() and (c32[:, 2] - c32[:, 0]).tobytes() == tree.tris["e1"].tobytes()
    assert np.array_equal(tree.tris["surface"], scene[0]["surface"][tree.tris["index"]]) and np.array_equal(tree.shade["surface"], scene[0]["surface"])


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_every_box_contains_its_padded_triangles(built, name):
    """For every leaf triangle and every slot on its path from the root: lo <= min corner - pad and hi >= max corner + pad, the
    right-hand sides formed in binary32 as the builder forms the padded box — no tolerance."""
    scene, tree = built[name]
    pad = expected_pad(scene)
    assert np.float32(tree.dump["pad"]).tobytes() == np.float32(pad).tobytes()
    slots = 0
    for node in range(tree.nodes.shape[0]):
        for k in range(4):
            ref = tree.ref[node, k]
            if ref == EMPTY:
                assert (tree.lo[node, k] == np.inf).all() and (tree.hi[node, k] == -np.inf).all()
                continue
            c = tree.corners[tree.tris["index"][tree.under(ref)]].reshape(-1, 3)
            assert c.shape[0] > 0
            assert (tree.lo[node, k] <= c.min(axis=0) - pad).all() and (tree.hi[node, k] >= c.max(axis=0) + pad).all(), (node, k)
            slots += 1
    assert slots > 0 or tree.tris.shape[0] == 0


def longest_path(tree, node=0):
    return 1 + max([longest_path(tree, c >> NODE_SHIFT) for c in tree.children(node) if not c & LEAF], default=0)


def deepest_stack(tree, node=0):
    """The most entries any descent leaves on the stack below `node`: entering one child leaves its siblings behind, whichever the order."""
    kids = tree.children(node)
    if not kids:
        return 0
    return len(kids) - 1 + max([deepest_stack(tree, c >> NODE_SHIFT) for c in kids if not c & LEAF], default=0)


EXPECTED_STACK = {"peel": 45, "peel_mirrored": 47, "none_hittable": 0}      # measured; the recursion above agrees


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_shape_and_stack(built, name):
    scene, tree = built[name]
    refs = tree.ref.reshape(-1)
    node_refs = refs[(refs != EMPTY) & ((refs & LEAF) == 0)]
    assert (node_refs % 64 == 0).all()
    parents = np.repeat(np.arange(tree.nodes.shape[0]), 4)[(refs != EMPTY) & ((refs & LEAF) == 0)]
    assert ((node_refs >> NODE_SHIFT) > parents).all()                                # children behind their parents
    assert np.array_equal(np.sort(node_refs >> NODE_SHIFT), np.arange(1, tree.nodes.shape[0]))     # every node referenced exactly once
    assert tree.dump["depth"] == longest_path(tree)
    if tree.tris.shape[0] == 0:
        assert tree.nodes.shape[0] == 1 and (refs == EMPTY).all() and tree.dump["stack_need"] == 0
    else:
        assert tree.dump["stack_need"] == deepest_stack(tree) + 1
    print("%s: %d nodes, depth %d, stack_need %d, skips set for %d of %d" % (
        name, tree.nodes.shape[0], tree.dump["depth"], tree.dump["stack_need"], int((tree.shade["skip_ref"] != EMPTY).sum()), tree.shade.shape[0]))
    assert tree.dump["stack_need"] <= STACK
    if name.startswith("peel"):
        assert tree.dump["stack_need"] >= 40
    if name in EXPECTED_STACK:
        assert tree.dump["stack_need"] == EXPECTED_STACK[name]


def effective_planes(tris):
    """Binary64 (unit normal, three effective vertices v0, v0 + e0, v0 + e1) of leaf-order triangles, from the stored binary32 edges."""
    v0, e0, e1 = (tris[f].astype(np.float64) for f in ("v0", "e0", "e1"))
    n = np.cross(e0, e1)
    return n / np.linalg.norm(n, axis=1, keepdims=True), np.stack([v0, v0 + e0, v0 + e1], 1)


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_a_skip_reference_covers_one_plane_only(built, name):
    """Every triangle under a triangle's skip_ref — itself included — lies within 1e-5 m of that triangle's plane, normals within 1e-3."""
    scene, tree = built[name]
    shade = tree.shade
    have = np.nonzero(shade["skip_ref"] != EMPTY)[0]
    assert (tree.leafpos[have] != 0xFFFFFFFF).all()
    assert (shade["skip_a"][have] >= np.float32(0.01)).all() and (shade["skip_a"][have] < 1).all() and (shade["skip_b"][have] >= 0).all()
    for ref in np.unique(shade["skip_ref"][have]):
        below = tree.under(ref)
        owners = have[shade["skip_ref"][have] == ref]
        assert np.isin(tree.leafpos[owners], below).all()                              # a triangle is below its own reference
        normal, verts = effective_planes(tree.tris[below])
        for pos in tree.leafpos[owners]:
            n, p = normal[np.nonzero(below == pos)[0][0]], verts[np.nonzero(below == pos)[0][0], 0]
            assert np.abs((verts - p) @ n).max() <= 1e-5, (name, ref)
            assert np.minimum(np.linalg.norm(normal - n, axis=1), np.linalg.norm(normal + n, axis=1)).max() <= 1e-3, (name, ref)


def test_skips_are_set_at_the_origin_and_stand_down_away_from_it(built):
    count = lambda name: int((built[name][1].shade["skip_ref"] != EMPTY).sum())
    assert count("grid_box") == 768 and count("room_768") == 768
    assert count("far_0") == 0 and count("far_1") == 0 and count("far_2") == 0 and count("far_3") == 0       # translated by 1e3 m and more
    assert count("stray_vertex") == 0                                                 # one far vertex that no triangle uses is enough


f32 = np.float32


def dot32(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross32(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def moeller_trumbore32(v0, e0, e1, o, d):
    """The reference's triangle test (kernel.cpp:62-88) on binary32 arrays, one rounding per operator: distances, 0 where it rejects."""
    pvec = cross32(d, e1)
    det = dot32(e0, pvec)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        invdet = f32(1) / det
        tvec = o - v0
        u = invdet * dot32(tvec, pvec)
        qvec = cross32(tvec, e0)
        v = invdet * dot32(d, qvec)
        t = invdet * dot32(e1, qvec)
    reject = ((det > f32(-EPSILON)) & (det < f32(EPSILON))) | (u < 0) | (u > 1) | (v < 0) | (v + u > 1)
    return np.where(reject, f32(0), t)


@pytest.mark.parametrize("name", ROOMS_WITH_SKIPS)
def test_the_skip_rule_never_hides_a_hit(built, name):
    """The rule itself, restated: a ray that starts at the binary32 hit point of a ray on triangle T and leaves with
    |dot(stored normal of T, d)| > skip_a + skip_b * t gets no distance above EPSILON from any triangle under T's skip_ref."""
    scene, tree = built[name]
    rng = np.random.default_rng(31)
    v = np.asarray(scene[1], np.float32)[:, :3]
    lo, hi = v.min(axis=0).astype(np.float64), v.max(axis=0).astype(np.float64)
    have = np.nonzero(tree.shade["skip_ref"] != EMPTY)[0]
    done = shallow = 0
    while done < 2000:
        T = int(rng.choice(have))
        rec = tree.tris[tree.leafpos[T]]
        a, b = rng.uniform(0, 1, 2)
        if a + b > 1:
            a, b = 1 - a, 1 - b
        target = rec["v0"].astype(np.float64) + a * rec["e0"] + b * rec["e1"]
        o_prev = (lo + (hi - lo) * rng.uniform(0.1, 0.9, 3)).astype(f32)
        d_prev = target - o_prev
        d_prev = (d_prev / np.linalg.norm(d_prev)).astype(f32)
        t = moeller_trumbore32(rec["v0"], rec["e0"], rec["e1"], o_prev, d_prev)
        if not t > f32(EPSILON):
            continue
        o = o_prev + d_prev * f32(t)
        d = rng.normal(size=3)
        d = (d / np.linalg.norm(d)).astype(f32)
        cos = abs(dot32(tree.shade["n"][T], d))
        if not cos > tree.shade["skip_a"][T] + tree.shade["skip_b"][T] * f32(t):
            shallow += 1
            continue
        below = tree.tris[tree.under(tree.shade["skip_ref"][T])]
        dist = moeller_trumbore32(below["v0"], below["e0"], below["e1"], o, d)
        assert not (dist > f32(EPSILON)).any(), (name, T, o, d, dist.max())
        done += 1
    assert shallow > 0                                                                  # both sides of the threshold were drawn


def test_refusals(tool, tmp_path):
    scene = E.tetrahedron()[0]
    far_vertex = scene[1].copy()
    far_vertex[1, 0] = 2.0 ** 30 + 128.0                                               # the next binary32 value above 2^30
    assert far_vertex[1, 0] > 2.0 ** 30
    dump = run_dump(tool, (scene[0], far_vertex, scene[2]), tmp_path / "coordinate")
    assert "2^30" in dump["error"] and dump["nodes"].shape[0] == 0 and dump["tris"].shape[0] == 0
    at_limit = scene[1].copy()
    at_limit[1, 0] = 2.0 ** 30                                                          # the documented limit itself is accepted
    assert run_dump(tool, (scene[0], at_limit, scene[2]), tmp_path / "limit")["error"] == ""
    for field, bad in (("v2", scene[1].shape[0]), ("surface", scene[2].shape[0])):
        triangles = scene[0].copy()
        triangles[field][3] = bad
        dump = run_dump(tool, (triangles, scene[1], scene[2]), tmp_path / field)
        assert "out of range" in dump["error"] and dump["nodes"].shape[0] == 0 and dump["tris"].shape[0] == 0
