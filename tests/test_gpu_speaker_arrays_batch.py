"""A 16-speaker layout through the batch entry points: the pipeline (rvb_pipeline_create over two contexts, and two one-context lanes
with two pairs per launch) and the two-shard rvb_multi with its exact-mode chain in three blocks — each against trace + merge +
configure + download on a lone context, bit for bit in RVB_IR_EXACT, within the re-ordered-sum bound in RVB_IR_FAST."""
import numpy as np
import pytest

from parallel_reverb_raytracer_amd import scenes
from parallel_reverb_raytracer_amd.dtypes import AIR_COEFFICIENTS

from test_gpu_speaker_arrays import fast_bound, oracle_ir, speakers_for

pytestmark = pytest.mark.gpu

NRAYS, NREFL = 512, 24
# (microphone, source) inside the cathedral's nave, clear of columns (z = +-6) and pews (y < 0.9)
PAIRS = [((14.0, 1.6, -0.9), (-18.0, 1.7, 0.7)), ((10.0, 1.5, 0.4), (-20.0, 2.0, -0.3)), ((-5.0, 1.8, 0.2), (20.0, 1.6, 0.5)),
         ((3.0, 2.5, -8.5), (-12.0, 1.7, 8.8)), ((22.0, 3.0, 9.0), (-24.0, 1.5, -9.2)), ((0.5, 12.0, 0.1), (16.0, 1.7, -0.6))]


@pytest.fixture(scope="module")
def rig():
    from parallel_reverb_raytracer_amd import capi
    scene, info = scenes.cathedral(3000)
    dirs = scenes.sphere_directions(NRAYS, seed=23)
    ctxs = [capi.Context(0) for _ in range(3)]
    for c in ctxs:
        c.set_scene(scene)
        c.set_directions(dirs)
    yield {"scene": scene, "info": info, "dirs": dirs, "lanes": ctxs[:2], "solo": ctxs[2]}
    for c in ctxs:
        c.close()


def _alone(solo, mic, src, directions, coefficients, mode):
    solo.trace(mic, src, NREFL, AIR_COEFFICIENTS)
    images = solo.get_raw_images(False)
    solo.ir_configure_speakers(mic, directions, coefficients, images=images)
    return solo.ir_download(True, 44100.0, mode), images


@pytest.mark.parametrize("layout", ["two_contexts", "two_lanes_two_pairs_per_launch"])
def test_pipeline_with_16_speakers_equals_a_lone_context(rig, layout):
    from parallel_reverb_raytracer_amd import capi
    directions, coefficients = speakers_for(16)
    a, b = rig["lanes"]
    pipe = capi.Pipeline([a, b]) if layout == "two_contexts" else capi.Pipeline(None, lanes=[[a], [b]], pairs_per_launch=2)
    try:
        pipe.configure_speakers(directions, coefficients, NREFL, AIR_COEFFICIENTS, 44100.0, True, capi.IR_EXACT)
        for mic, src in PAIRS:
            pipe.submit(mic, src)
        got = [pipe.next() for _ in PAIRS]
        assert pipe.pending() == 0
    finally:
        pipe.close()
    seen = set()
    for k, (hist, info) in enumerate(got):
        want, images = _alone(rig["solo"], PAIRS[k][0], PAIRS[k][1], directions, coefficients, capi.IR_EXACT)
        assert info["job"] == k and info["images"] == images.shape[0]
        assert hist.shape == want.shape and hist.shape[0] == 16 and np.array_equal(hist, want) and hist.any(), k
        seen.add(hist.tobytes())
    assert len(seen) == len(PAIRS)                    # six different impulse responses


def test_multi_with_16_speakers_over_two_shards(rig, oracle):
    from parallel_reverb_raytracer_amd import capi
    directions, coefficients = speakers_for(16)
    mic, src = rig["info"]["mic"], rig["info"]["source"]
    want, images = _alone(rig["solo"], mic, src, directions, coefficients, capi.IR_EXACT)
    all_raw = np.concatenate([rig["solo"].get_raw_diffuse(), images])
    m = capi.MultiContext([0, 0])
    try:
        m.set_scene(rig["scene"])
        m.set_chain_blocks(3)
        m.raytrace(mic, src, rig["dirs"], NREFL, AIR_COEFFICIENTS)
        exact = m.ir_speakers(mic, directions, coefficients, True, 44100.0, capi.IR_EXACT)
        fast = m.ir_speakers(mic, directions, coefficients, True, 44100.0, capi.IR_FAST)
    finally:
        m.close()
    assert exact.shape == want.shape and exact.shape[0] == 16 and np.array_equal(exact, want) and exact.any()
    _, nb, chans = oracle_ir(oracle, mic, all_raw, directions, coefficients, True, 44100.0)
    assert fast.shape == exact.shape and nb == exact.shape[2] and fast.any()
    assert (np.abs(fast.astype(np.float64) - exact) <= fast_bound(exact, chans, 44100.0)).all()
