"""One context, used for a long time: the directed sequences and the seeded walks of tests/context_model.py on ONE capi.Context that
lives for the whole module, against the model's answer after every operation — the error code of a refused call, or the bytes of the
CPU oracle (records, direct slot, candidates, time range, materialised attenuation, flatten and RVB_IR_EXACT histograms bit for bit,
padding included; RVB_IR_FAST within fast_bound of tests/test_gpu_speaker_arrays.py).  tests/test_context_model_host.py shows without a
GPU that these walks notice every invalidation the context's code could forget.

A failure prints the walk up to the failing step in the form replay() takes: paste the list into DIRECTED of tests/context_model.py to
keep it as a named case."""
import ctypes

import numpy as np
import pytest

import context_model as cm
from parallel_reverb_raytracer_amd.dtypes import ATTENUATED, IMPULSE

pytestmark = pytest.mark.gpu


def walk_context():
    from parallel_reverb_raytracer_amd import capi

    class WalkContext(capi.Context):
        """capi.Context, the two halves of rvb_flatten as calls of their own, rvb_ir_time_range_begin, and fetches into buffers that
        hold the largest trace of the menus whatever the context believes to hold."""

        def get_raw_diffuse(self):
            out = np.zeros(cm.MAX_RECORDS, dtype=IMPULSE)
            self._check(self.lib.rvb_get_diffuse(self.handle, out.ctypes.data_as(ctypes.c_void_p)))
            return out

        def _flatten(self, attenuated, sample_rate, out, capacity):
            assert attenuated.dtype == ATTENUATED and attenuated.flags.c_contiguous
            nbins = ctypes.c_uint64(0)
            self._check(self.lib.rvb_flatten(self.handle, attenuated.ctypes.data_as(ctypes.c_void_p), attenuated.shape[0], sample_rate,
                                             out.ctypes.data_as(ctypes.c_void_p) if out is not None else None, capacity, ctypes.byref(nbins)))
            return int(nbins.value)

        def flatten_query(self, attenuated, sample_rate):
            return self._flatten(attenuated, sample_rate, None, 0)

        def flatten_fill(self, attenuated, sample_rate, capacity):
            out = np.zeros((8, capacity), dtype=np.float32)
            assert self._flatten(attenuated, sample_rate, out, capacity) == capacity
            return out

        def ir_accumulate_tensor(self, predelay, sample_rate, nbins, mode, tensor):
            """(as the parent's, for a tensor that may hold more rows than the context has channels: a refused call gets a real buffer)"""
            assert tensor.is_cuda and tensor.is_contiguous() and tensor.numel() >= self.nchannels * 8 * nbins
            self.ir_accumulate_wait_for_torch()
            self.ir_accumulate(predelay, sample_rate, nbins, mode, tensor.data_ptr())

        def ir_exact_fold_tensor(self, nbins, bin_begin, bin_end, tensor):
            assert tensor.is_cuda and tensor.is_contiguous() and tensor.numel() >= self.nchannels * 8 * nbins
            self.ir_accumulate_wait_for_torch()
            self._check(self.lib.rvb_ir_exact_fold(self.handle, nbins, bin_begin, bin_end, tensor.data_ptr()))

        def ir_time_range_begin(self):
            self._check(self.lib.rvb_ir_time_range_begin(self.handle))

    return WalkContext(0)          # raises when librvb_hip.so or the GPU is missing: no fallback


@pytest.fixture(scope="module")
def world(oracle):
    return cm.World(oracle)


class Lifetime:
    """The module's one context, the model that follows it from its creation and every operation both have seen.  A walk starts where
    the walks before it left them.  After a disagreement the model no longer describes the context: both are replaced, so that the
    tests that follow fail only for reasons of their own, and the failure's list holds the whole life of the context it happened on."""

    def __init__(self, world):
        self.world, self.ctx = world, None
        self.renew()

    def renew(self):
        if self.ctx is not None:
            self.ctx.close()
        self.ctx, self.model, self.history = walk_context(), cm.ContextModel(self.world), []

    def replay(self, ops, label, **more):
        try:
            walk = cm.replay(self.world, self.ctx, "cuda", ops, label, model=self.model, before=self.history, **more)
        except BaseException:
            self.renew()
            raise
        self.history.extend(walk.ops)
        return walk


@pytest.fixture(scope="module")
def ctx(world):
    life = Lifetime(world)
    yield life
    life.ctx.close()


def replay(world, ops, label="replay"):
    """Runs a list of operations, as a failing walk prints it, on a context and a model of its own."""
    c = walk_context()
    try:
        return cm.replay(world, c, "cuda", ops, label)
    finally:
        c.close()


@pytest.mark.parametrize("name", list(cm.DIRECTED))
def test_directed_sequence(world, ctx, name):
    walk = ctx.replay(cm.DIRECTED[name], "directed sequence " + name, keep_histograms="on_top" in name)
    if "on_top" in name:
        assert cm.on_top_is_the_all_chain(walk)


@pytest.mark.parametrize("seed", cm.SEEDS)
def test_seeded_walk(world, ctx, seed):
    ctx.replay(cm.seeded_walk(seed), "seed %d" % seed)
