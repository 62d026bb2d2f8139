"""The constructed room of tests/image_edges.py holds what it is built for (CPU oracle only, no GPU), so that no test of
tests/test_gpu_image_edges.py passes on empty ground: image sources of every order 1 .. 9 in every pair, with and without the hole;
(ray, order) items that pass the plan kernel's crossing test and are rejected by a closest-hit or visibility query; rays whose rejected
order is followed by a valid one; a visible and two hidden direct paths; escaping rays; chains that die in one band under table B.

An item is REJECTED BY A QUERY when it is valid in the room without the panel, invalid with the panel, and the ray's first `order`
diffuse records (position and time, bit for bit) are the same in both rooms: the crossing test depends only on the triangles the ray
hit, the microphone and the source, so with the panel it passes as it does without, and what rejects the item is a query."""
import numpy as np
import pytest

import image_edges as E
from parallel_reverb_raytracer_amd.dtypes import NUM_IMAGE_SOURCE

NRAYS, NREFL = E.MAIN
ORDERS = NUM_IMAGE_SOURCE - 1


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def traced(oracle):
    """(panel, hole, pair, table name) -> the oracle's (diffuse, image, index) at 509 x 12, computed once"""
    done = {}
    tables = E.tables()

    def get(panel, hole, pair, table="A"):
        key = (panel, hole, pair, table)
        if key not in done:
            surfaces, air = tables[table]
            mic, source = E.PAIRS[pair]
            done[key] = oracle.raytrace(E.with_table(E.room(panel, hole), surfaces), mic, source, E.directions(NRAYS), NREFL, air)
        return done[key]
    return get


def valid_orders(index, nrays=NRAYS):
    """[nrays][9]: the ray has an image source of order 1 + column"""
    return index.reshape(nrays, NUM_IMAGE_SOURCE)[:, 1:] != 0


def rejected_by_a_query(with_panel, without_panel, nrays=NRAYS, nrefl=NREFL):
    """[nrays][9] of the definition above, from two oracle traces"""
    a, b = with_panel[0].reshape(nrays, nrefl), without_panel[0].reshape(nrays, nrefl)
    same = (bits(a["position"]) == bits(b["position"])).all(axis=2) & (bits(a["time"]) == bits(b["time"]))
    prefix = np.logical_and.accumulate(same, axis=1)                 # [ray][k]: the records 0 .. k agree
    last = min(nrefl, ORDERS)
    out = np.zeros((nrays, ORDERS), bool)
    out[:, :last] = (valid_orders(without_panel[2], nrays) & ~valid_orders(with_panel[2], nrays))[:, :last] & prefix[:, :last]
    return out


@pytest.mark.parametrize("hole", [False, True])
@pytest.mark.parametrize("pair", [0, 1, 2])
def test_every_order_has_candidates(traced, pair, hole):
    per_order = valid_orders(traced(True, hole, pair)[2]).sum(axis=0)
    print("pair", pair, "hole", hole, "valid candidates per order 1..9:", per_order.tolist())
    assert (per_order >= 3).all()


def test_items_rejected_by_a_query(traced):
    third = rejected_by_a_query(traced(True, False, 2), traced(False, False, 2)).sum(axis=0)
    second = rejected_by_a_query(traced(True, False, 1), traced(False, False, 1)).sum(axis=0)
    print("query-rejected items per order 1..9, pair three:", third.tolist(), "pair two:", second.tolist())
    assert (third[:7] >= 1).all() and third.sum() >= 15
    assert second[0] >= 50


def test_a_rejected_order_is_followed_by_a_valid_one(traced):
    for pair in (1, 2):
        rejected = rejected_by_a_query(traced(True, False, pair), traced(False, False, pair))
        valid = valid_orders(traced(True, False, pair)[2])
        later = np.flip(np.logical_or.accumulate(np.flip(valid, 1), axis=1), 1)          # [ray][k]: an order >= k + 1 is valid
        rays = (rejected[:, :-1] & later[:, 1:]).any(axis=1).sum()
        print("pair", pair, "rays with a query-rejected order and a valid higher one:", int(rays))
        assert rays >= 1


@pytest.mark.parametrize("hole", [False, True])
def test_direct_paths(traced, hole):
    for pair, visible in enumerate(E.DIRECT_VISIBLE):
        direct = traced(True, hole, pair)[1][:1]
        if visible:
            assert (direct["volume"] != 0).all() and direct["time"][0] > 0
        else:
            assert not direct.view(np.uint32).any(), "the direct path of pair %d is not hidden" % pair
            assert (traced(False, hole, pair)[1][:1]["volume"] != 0).all(), "... or hidden by something else than the panel"


def test_rays_escape_through_the_hole(traced):
    for pair in range(3):
        empty = ~traced(True, True, pair)[0].view(np.uint32).reshape(NRAYS, NREFL, 16).any(axis=2)
        escaped = empty[:, :ORDERS].any(axis=1).sum()
        print("pair", pair, "rays that escape within nine bounces:", int(escaped))
        assert 100 <= escaped < NRAYS
        assert traced(True, False, pair)[0].view(np.uint32).reshape(NRAYS * NREFL, 16).any(axis=1).all(), "a ray leaves the closed room"


def test_merged_images(oracle, traced):
    for pair in range(3):
        _, image, index = traced(True, False, pair)
        merged = oracle.collect_images(image, index, False)
        print("pair", pair, "merged images:", merged.shape[0], "of", int(valid_orders(index).sum()), "candidates")
        assert merged.shape[0] >= 100
        assert valid_orders(index).sum() >= 2 * merged.shape[0], "hardly any key has more than one ray"


def test_table_b(oracle, traced):
    a_table, b_table = E.tables()["A"][0], E.tables()["B"][0]
    assert (a_table["specular"] != b_table["specular"]).all() and (a_table["diffuse"] != b_table["diffuse"]).all()
    assert b_table["specular"][E.DEAD_SURFACE][E.DEAD_BAND] == 0 and not b_table["diffuse"][E.MUTE].any()
    assert len({tuple(row) for row in a_table["specular"].T.tolist()}) == 8 and len({tuple(row) for row in a_table["specular"].tolist()}) == E.NSURFACES
    live = [b for b in range(8) if b != E.DEAD_BAND]
    for pair in range(3):
        (_, image_a, index_a), (_, image_b, index_b) = traced(True, False, pair, "A"), traced(True, False, pair, "B")
        assert np.array_equal(index_a, index_b)
        a, b = oracle.collect_images(image_a, index_a, True), oracle.collect_images(image_b, index_b, True)
        assert a.shape == b.shape and np.array_equal(bits(a["position"]), bits(b["position"]))
        assert (a["volume"][:, live] != b["volume"][:, live]).all()
        dead = b["volume"][:, E.DEAD_BAND] == 0
        # the order of a merged image: that of the candidates at its position (an image source of order k lies behind k mirrors)
        cand = image_b.reshape(NRAYS, NUM_IMAGE_SOURCE)[:, 1:][valid_orders(index_b)]
        order = np.nonzero(valid_orders(index_b))[1] + 1
        orders_of_dead = {int(k) for p in b["position"][dead] for k in order[(bits(cand["position"]) == bits(p)).all(axis=1)]}
        negative = (np.signbit(b["volume"][:, E.DEAD_BAND]) & dead).sum()
        print("pair", pair, "merged images with a zero in the dead band:", int(dead.sum()), "of", b.shape[0], "(-0: %d)" % negative, "orders", sorted(orders_of_dead))
        assert dead.any() and not dead.all() and orders_of_dead and min(orders_of_dead) >= 2
        assert (a["volume"] != 0).all() and (b["volume"][dead][:, live] != 0).all()
        # the diffuse records: some lose all their volume on the mute wall, the others change
        da, db = traced(True, False, pair, "A")[0], traced(True, False, pair, "B")[0]
        live_a, live_b = (da["volume"] != 0).any(axis=1), (db["volume"] != 0).any(axis=1)
        assert (live_a & ~live_b).any() and (live_a & live_b).any()


def test_the_other_microphones(traced, oracle):
    """What the relisten tests move to: pair one's source heard from the microphones of pairs two and three, and every pair's source from
    the next pair's microphone.  Each has candidates of every order and a query-rejected item."""
    dirs = E.directions(NRAYS)
    for source, mic in ((0, 1), (0, 2), (1, 2), (2, 0)):
        with_panel = oracle.raytrace(E.room(), E.PAIRS[mic][0], E.PAIRS[source][1], dirs, NREFL, E.tables()["A"][1])
        without = oracle.raytrace(E.room(False), E.PAIRS[mic][0], E.PAIRS[source][1], dirs, NREFL, E.tables()["A"][1])
        per_order, rejected = valid_orders(with_panel[2]).sum(axis=0), rejected_by_a_query(with_panel, without).sum()
        print("source", source, "microphone", mic, "valid per order:", per_order.tolist(), "query-rejected:", int(rejected))
        assert (per_order >= 3).all() and rejected >= 1


@pytest.mark.parametrize("offset", [0, 5, E.RAY_OFFSET])
def test_get_pair_candidates_under_a_ray_offset(oracle, traced, offset):
    """capi.Context.get_pair_candidates is host code over the reported rays (offset + pair * nrays + ray); tests/oracle_tracer.py shares
    it.  Whatever the trace's ray offset, every pair gets its own candidates, ray numbers relative to the pair."""
    from oracle_tracer import OracleTracer
    tracer = OracleTracer(oracle, E.room(), E.directions(NRAYS))
    tracer.trace_pairs(E.MICS, E.SOURCES, NREFL, E.tables()["A"][1], ray_offset=offset)
    reported = tracer.get_image_candidates()
    assert reported["ray"].min() >= offset and reported["ray"].max() < offset + 3 * NRAYS
    for pair in range(3):
        rays, slots = np.nonzero(valid_orders(traced(True, False, pair)[2]))
        mine = tracer.get_pair_candidates(pair, reported)
        assert mine.shape[0] == rays.shape[0], (pair, mine.shape[0], rays.shape[0])
        assert np.array_equal(mine["ray"].astype(np.int64), rays) and np.array_equal(mine["slot"].astype(np.int64), slots + 1)


@pytest.mark.parametrize("nrays,nrefl", E.EDGE_SHAPES)
def test_edge_shapes(oracle, nrays, nrefl):
    """Every order the shape can have (min(nreflections, 9)) is there at 64 and 130 rays; five rays reach order 2 at least."""
    mic, source = E.PAIRS[0]
    for hole in (False, True):
        _, _, index = oracle.raytrace(E.room(True, hole), mic, source, E.directions(nrays), nrefl, E.tables()["A"][1])
        per_order = valid_orders(index, nrays).sum(axis=0)
        print(nrays, nrefl, "hole", hole, "valid per order:", per_order.tolist())
        last = min(nrefl, ORDERS)
        assert not per_order[last:].any()
        assert (per_order[:last] >= 1).all() if nrays >= 64 else (per_order[:2] >= 1).all()
