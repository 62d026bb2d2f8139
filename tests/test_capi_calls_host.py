"""What capi.py passes to librvb_hip.so, call by call: a recording stand-in takes the place of the loaded library (Context.lib,
MultiContext.lib, Pipeline.lib, the module's _lib), every public method of the three handle classes and merge_images are driven once
per branch that changes the symbol called or which arguments are null, and the log must equal tests/golden/capi_calls.txt line for
line.  No GPU is opened and the shared library is not loaded.

A line is the symbol and then every argument in a canonical form that the HEADER's prototype of the symbol decides (capi_header.py),
so that a hand-wrapped ctypes.c_float(x) and a bare x under argtypes log the same:
  - a scalar parameter: the value after conversion through its C type (float through c_float); an integer parameter takes what the
    ctypes integer types take (a bool or a numpy integer, not 7.0), and a bare Structure where a pointer is due is refused, as
    argtypes refuse them in the real library;
  - a pointer parameter: `null`; the bytes in hex of a ctypes array or Structure (`ref:` in front when it came through byref; bytes
    beyond 64 as a length and a CRC); `ptr:<itemsize>x<count>:<crc32>` for a numpy array that went through capi._ptr;
    `ptr:<name>` for an address this test handed in (handles, stand-in tensors, the stand-in event); `ptr` for anything else.
The stand-in returns RVB_OK and fills the out-parameters a method needs to go on (a handle, a count, nbins, a pipeline result).

    python tests/test_capi_calls_host.py [--capi <path to another capi.py>] [--write]

holds the log of another capi.py (e.g. an earlier commit's, saved to a file) against the fixture; --write records it anew, which
is right only when a call into the library is changed on purpose.

NOT PINNED, because they need torch on a device; each is called by a GPU test:
  - Context.reshade_grad_map(out=None), the torch.empty of the map: tests/test_gpu_reshade_grad_map.py::test_decay_sensitivity_map
    (through fitting.decay_sensitivity_map);
  - Context.decay_curve_tensor(curve=None), the torch.empty_like of the curve: tests/test_gpu_decay.py and the decay fit tests.
Both are pinned here with the tensor given, which is the same call into the library."""
import ctypes
import importlib.util
import operator
import os
import sys
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from capi_header import ROOT, prototypes  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "capi_calls.txt")
CAPI = os.path.join(ROOT, "parallel-reverb-raytracer_amd", "capi.py")
SCALARS = {"int": ctypes.c_int, "unsigned": ctypes.c_uint, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "float": ctypes.c_float}
BASE = 1 << 32          # the addresses this test invents lie above 4 GiB: a value cut to 32 bits would lose its name


def _hex(obj):
    raw = bytes(memoryview(obj).cast("B")) if not isinstance(obj, ctypes._SimpleCData) else ctypes.string_at(ctypes.addressof(obj), ctypes.sizeof(obj))
    return raw.hex() if len(raw) <= 64 else "%dB:%08x" % (len(raw), zlib.crc32(raw))


class Recorder:
    """Stands in for the loaded library: any rvb_* attribute is a function that logs its call and returns RVB_OK."""

    def __init__(self):
        self.protos = {name: (ret, params) for name, ret, params in prototypes()}
        self.lines, self.names, self.keep, self.handles = [], {}, [], 0
        self.histogram = (ctypes.c_float * (2 * 8 * 3))(*range(48))
        self.returns = {"rvb_ir_bins": 7, "rvb_pipeline_pending": 2, "rvb_multi_used_rccl": 1, "rvb_multi_peer_links": 3}
        # symbol -> {argument index: value for the out-parameter}
        self.fills = {"rvb_create": {0: self.handle}, "rvb_multi_create": {0: self.handle}, "rvb_pipeline_create": {0: self.handle},
                      "rvb_pipeline_create_lanes": {0: self.handle}, "rvb_merge_images": {6: 3}, "rvb_get_image_candidates": {3: 2},
                      "rvb_flatten": {6: 5}, "rvb_ir_download": {6: 5}, "rvb_multi_get_images": {4: 3}, "rvb_multi_ir_speakers": {11: 4},
                      "rvb_multi_ir_hrtf": {12: 4}, "rvb_multi_context": {3: 100, 4: 28},
                      "rvb_pipeline_next": {1: {"job": 9, "histogram": ctypes.cast(self.histogram, ctypes.POINTER(ctypes.c_float)), "nchannels": 2,
                                                "nbins": 3, "predelay": 0.25, "max_time": 1.5, "nimages": 6}}}

    def handle(self):
        self.handles += 1
        self.names[BASE + self.handles * 0x1000] = "ptr:handle%d" % self.handles
        return BASE + self.handles * 0x1000

    def address(self, name):
        addr = BASE + 0x100000 * (1 + len(self.names))
        self.names[addr] = "ptr:" + name
        return addr

    def numpy_pointer(self, a):
        """capi._ptr, and the array remembered by its address (and kept, so that the address is not used again)."""
        if a is None:
            return None
        self.keep.append(a)
        self.names[a.ctypes.data] = "ptr:%dx%d:%08x" % (a.dtype.itemsize, a.size, zlib.crc32(a.tobytes()))
        return a.ctypes.data_as(ctypes.c_void_p)

    def _pointer(self, a):
        if a is None:
            return "null"
        if hasattr(a, "_obj"):
            return "ref:" + _hex(a._obj)
        assert not isinstance(a, ctypes.Structure), "a bare Structure where the library takes a pointer: pass byref"     # as c_void_p refuses it
        if isinstance(a, ctypes.Array):
            return _hex(a)
        addr = a.value if isinstance(a, ctypes._SimpleCData) else int(a)
        return self.names.get(addr, "ptr") if addr else "null"

    def _scalar(self, kind, a):
        v = a.value if isinstance(a, ctypes._SimpleCData) else a
        # integers as the ctypes integer types take them: 7.0 is a TypeError, a bool or a numpy integer passes
        return repr(SCALARS[kind](float(v) if kind == "float" else operator.index(v)).value)

    def __getattr__(self, symbol):
        if not symbol.startswith("rvb_"):
            raise AttributeError(symbol)
        ret, params = self.protos[symbol]

        def call(*args):
            assert len(args) == len(params), "%s: %d arguments, the header declares %d" % (symbol, len(args), len(params))
            self.lines.append(" ".join([symbol] + [self._pointer(a) if k in ("pointer", "const char *") else self._scalar(k, a) for k, a in zip(params, args)]))
            for index, value in self.fills.get(symbol, {}).items():
                if args[index] is None:
                    continue
                target = args[index]._obj
                if isinstance(value, dict):
                    for field, v in value.items():
                        setattr(target, field, v)
                else:
                    target.value = value() if callable(value) else value
            return self.returns.get(symbol, b"" if ret == "const char *" else None if ret == "void" else 0)
        return call


class Tensor:
    """What the tensor methods read of a torch CUDA tensor, and nothing else."""
    is_cuda = True

    def __init__(self, rec, name, shape, pinned=False):
        import torch
        self.dtype, self.shape, self._pinned, self._addr = torch.float32, tuple(shape), pinned, rec.address(name)

    def is_contiguous(self):
        return True

    def is_pinned(self):
        return self._pinned

    def numel(self):
        return int(np.prod(self.shape))

    def element_size(self):
        return 4

    def dim(self):
        return len(self.shape)

    def data_ptr(self):
        return self._addr


def load(path):
    """capi.py at `path` as a module of its own inside the package (its relative imports work), library stand-in installed."""
    sys.path.insert(0, ROOT)
    import rvb_import
    rvb_import.load()
    name = rvb_import.PACKAGE_NAME + "._capi_under_pin"
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    rec = Recorder()
    mod._lib, mod.load_library, mod._ptr = rec, lambda: rec, rec.numpy_pointer
    return mod, rec


def drive(mod, rec):
    from parallel_reverb_raytracer_amd import scenes
    from parallel_reverb_raytracer_amd.dtypes import AIR_COEFFICIENTS as air, ATTENUATED, IMPULSE

    def section(title):
        rec.lines.append("# " + title)

    scene = scenes.rotated_square_room(n=4)
    dirs = scenes.sphere_directions(8, seed=5)
    mic, src, facing, up = (0.0, 2.0, 0.5), (0.25, 2.0, 2.0), (0.0, 0.0, 1.0), (0.0, 1.0, 0.0)
    source_table = (np.arange(360 * 180 * 8, dtype=np.float32) % 7).reshape(360, 180, 8)
    hrtf = (np.arange(2 * 360 * 180 * 8, dtype=np.float32) % 11).reshape(2, 360, 180, 8)
    impulses = np.zeros(3, dtype=IMPULSE)
    impulses["time"] = [0.5, 0.25, 0.125]
    cand = np.zeros(3, dtype=mod.IMAGE_CANDIDATE)
    cand["ray"], cand["slot"], cand["index"] = [5, 2, 2], [3, 3, 1], [7, 7, 9]

    section("merge_images")
    mod.merge_images(cand, impulses[:1], True)
    mod.merge_images(cand, None, 0)

    section("Context: scene, rays, traces")
    ctx, other = mod.Context(0), mod.Context(3)
    ctx.set_scene(scene)
    other.share_scene(ctx)
    ctx.scene_info()
    ctx.device_info()
    ctx.set_directions(dirs)
    ctx.set_directions_device(rec.address("directions"), 8)
    other.set_directions(dirs)
    mod.Context.trace_group([ctx, other], [mic, src], [src, mic], 16, air)
    mod.Context.trace_group([ctx, other], [mic, src], [src, mic], 16, air, ray_offsets=[8, np.int64(16)])
    ctx.set_concurrent_traces(np.int64(3))
    ctx.set_path_lanes(True)
    ctx.set_source_pattern(None)
    ctx.set_source_pattern((0.0, 0.0, 1.0), None)
    ctx.set_source_pattern((0.0, 0.0, 1.0), 0.5)
    ctx.set_source_pattern([(0.0, 0.0, 1.0), (1.0, 0.0, 0.0)], [[0.5] * 8, [0.25] * 8])
    ctx.set_source_table(None)
    ctx.set_source_table(source_table, facing, up)
    ctx.set_source_table(source_table, [facing, up], up)
    ctx.keep_paths(False)
    ctx.keep_paths(True)
    ctx.keep_paths(True, listener=True)
    ctx.trace(mic, src, 16, air)
    ctx.trace(mic, src, np.int64(16), air, ray_offset=24)
    ctx.trace_pairs([mic, src], [src, mic], 16, air, ray_offset=8)
    ctx.select_pair(1)
    ctx.raytrace(mic, src, dirs, 16, air)
    ctx.relisten([src])
    ctx.reshade(None, air)
    ctx.reshade(scene[2], air)
    ctx.reshade_grad(0.125, 44100.0, 77, rec.address("grad_weights"))
    ctx.reshade_grad_map(0.125, 44100.0, 77, rec.address("map_weights"), out=Tensor(rec, "map", (ctx.ntriangles, 16)))
    ctx.synchronize()

    section("Context: raw results")
    ctx.get_raw_diffuse()
    ctx.diffuse_device()
    ctx.get_direct()
    ctx.get_image_candidates()
    ctx.get_pair_candidates(0)
    ctx.get_raw_images(True)
    ctx.get_all_raw(False)
    rec.fills["rvb_get_image_candidates"] = {3: 0}
    ctx.get_image_candidates()
    rec.fills["rvb_get_image_candidates"] = {3: 2}
    bare = mod.Context(1)
    bare.get_raw_images(False)                     # no rays set: no direct impulse
    bare.close()
    ctx.executed_bounces()
    ctx.debug_stamps()
    ctx.last_timings()

    section("Context: materialised attenuators")
    ctx.attenuate_speaker(mic, impulses, (1.0, 0.0, -1.0), 0.5)
    ctx.attenuate_speaker_device(mic, rec.address("d_in"), 3, (1.0, 0.0, -1.0), 0.5, rec.address("d_out"))
    ctx.attenuate_hrtf_device(mic, rec.address("d_in2"), 3, hrtf[1], facing, up, 1, rec.address("d_out2"))
    ctx.attenuate_hrtf(mic, impulses, hrtf[0], facing, up, 0)
    ctx.flatten(np.zeros(3, dtype=ATTENUATED), 44100.0)

    section("Context: fused impulse responses")
    ctx.ir_configure_speakers(mic, [(-1, 0, -1), (1, 0, -1)], [0.5, 0.25])
    ctx.ir_configure_speakers(mic, [(-1, 0, -1), (1, 0, -1)], [0.5, 0.25], which=mod.IR_DIFFUSE, images=impulses)
    ctx.ir_configure_hrtf(mic, hrtf, facing, up)
    ctx.ir_configure_hrtf(mic, None, facing, up, which=mod.IR_IMAGES, images=impulses)
    ctx.ir_time_range()
    ctx.ir_bins(1.5, 0.25, 44100.0)
    ctx.ir_accumulate(0.25, 44100.0, 7, mod.IR_EXACT, rec.address("histogram"))
    histogram, pinned = Tensor(rec, "histogram_tensor", (2, 8, 7)), Tensor(rec, "pinned_tensor", (2, 8, 7), pinned=True)
    ctx.ir_accumulate_wait_for_torch()
    ctx.ir_accumulate_tensor(0.25, 44100.0, 7, mod.IR_FAST, histogram)
    ctx.ir_accumulate_export_tensor(0.25, 44100.0, 7, mod.IR_EXACT, histogram, pinned)
    ctx.ir_accumulate_export_tensor(0.25, 44100.0, 7, mod.IR_EXACT, histogram, pinned, slices=np.int32(4))
    ctx.ir_exact_prepare(0.25, 44100.0, 7)
    ctx.ir_exact_fold_tensor(7, 2, 5, histogram)
    ctx.export_tensor_to_host(histogram, pinned)
    ctx.synchronize_exports()
    ctx.ir_download(True, 44100.0)
    ctx.ir_download(np.bool_(False), 48000.0, mod.IR_EXACT)

    section("Context: decay")
    h, e, t, m, w = (rec.address("decay_" + n) for n in ("histogram", "curve", "target", "mask", "weights"))
    ctx.decay_curve(h, 16, 7, e)
    ctx.decay_times(e, 16, 7, 44100.0)
    ctx.decay_times(e, np.int64(16), 7, 44100.0, 0.0, -10.0)
    ctx.decay_loss(h, e, t, m, 16, 7)
    ctx.decay_loss(h, e, t, m, 16, 7, flags=np.uint32(0), device_weights_pointer=w)
    ctx.decay_params(e, 16, 7, 44100.0)
    targets, weights = np.full((16, 7), 0.5, dtype=np.float32), np.ones((16, 7), dtype=np.float32)
    ctx.decay_params_loss(h, e, 16, 7, 44100.0, targets, weights)
    ctx.decay_params_loss(h, e, 16, 7, 44100.0, targets, weights, device_weights_pointer=w)
    th, te, tt, tm, tw = (Tensor(rec, "tensor_" + n, (2, 8, 7)) for n in ("histogram", "curve", "target", "mask", "weights"))
    ctx.decay_curve_tensor(th, te)
    ctx.decay_times_tensor(te, 44100.0)
    ctx.decay_loss_tensor(th, te, tt, tm)
    ctx.decay_loss_tensor(th, te, tt, tm, flags=0, weights=tw)
    ctx.decay_params_tensor(te, 44100.0)
    ctx.decay_params_loss_tensor(th, te, 44100.0, targets, weights)
    ctx.decay_params_loss_tensor(th, te, 44100.0, targets, weights, weights=tw)

    section("MultiContext")
    multi = mod.MultiContext([0, np.int64(2)], flags=mod.MULTI_REHEARSE_RCCL)
    multi.set_scene(scene)
    multi.raytrace(mic, src, dirs, 16, air)
    multi.set_source_pattern(None)
    multi.set_source_pattern((0.0, 0.0, 1.0), [0.5] * 8)
    multi.shard(1)
    multi.used_rccl()
    multi.set_chain_blocks(np.int64(4))
    multi.peer_links()
    multi.get_raw_diffuse()
    multi.get_raw_images(True)
    multi.ir_speakers(mic, [(-1, 0, -1), (1, 0, -1)], [0.5, 0.25], True, 44100.0, mod.IR_EXACT)
    multi.ir_speakers(mic, [(-1, 0, -1)], [0.5], False, 48000.0, mod.IR_FAST, which=mod.IR_DIFFUSE, remove_direct=True)
    multi.ir_hrtf(mic, hrtf, facing, up, True, 44100.0, mod.IR_EXACT)
    multi.ir_hrtf(mic, hrtf, facing, up, False, 48000.0, mod.IR_FAST, which=mod.IR_IMAGES, remove_direct=True)
    multi.close()
    multi.close()                                  # a closed handle is not destroyed twice

    section("Pipeline")
    pipe = mod.Pipeline([ctx, other], group=2)
    pipe.configure_speakers([(-1, 0, -1), (1, 0, -1)], [0.5, 0.25], 16, air)
    pipe.configure_speakers([(-1, 0, -1)], [0.5], 16, air, sample_rate=48000.0, trim_predelay=False, mode=mod.IR_FAST, which=mod.IR_DIFFUSE, remove_direct=True)
    pipe.configure_hrtf(hrtf, facing, up, 16, air)
    pipe.configure_hrtf(hrtf, facing, up, 16, air, sample_rate=48000.0, trim_predelay=False, mode=mod.IR_FAST, which=mod.IR_IMAGES, remove_direct=True)
    pipe.set_source_pattern(None)
    pipe.set_source_pattern((0.0, 0.0, 1.0), 0.5)
    pipe.submit(mic, src)
    pipe.submit(mic, src, facing, up)
    pipe.submit(mic, src, source_direction=(1.0, 0.0, 0.0))
    pipe.submit(mic, src, facing, up, source_direction=(1.0, 0.0, 0.0))
    pipe.pending()
    histogram, info = pipe.next()
    rec.lines.append("# next: %s %s" % (histogram.shape, sorted(info.items())))
    pipe.next(copy=False)
    pipe.close()
    lanes = mod.Pipeline(None, group=np.int64(1), lanes=[[ctx], [other]], pairs_per_launch=np.int64(2))
    rec.lines.append("# limit %d valid_for %d" % (lanes.limit, lanes.valid_for))
    lanes.close()
    mod.Pipeline([ctx, other], pairs_per_launch=4).close()

    section("close")
    ctx.close()
    ctx.close()
    other.close()
    return "\n".join(rec.lines) + "\n"


class Event:
    """Stands in for torch.cuda.Event: record() and the address of the HIP event."""
    address = None

    def record(self):
        pass

    @property
    def cuda_event(self):
        return Event.address


def record(path=CAPI):
    import torch
    mod, rec = load(path)
    Event.address = rec.address("event")
    real, torch.cuda.Event = torch.cuda.Event, Event
    try:
        return drive(mod, rec)
    finally:
        torch.cuda.Event = real


def compare(got):
    with open(FIXTURE) as f:
        want = f.read().splitlines()
    got = got.splitlines()
    for k, (a, b) in enumerate(zip(got, want)):
        assert a == b, "line %d: %r, recorded %r" % (k + 1, a, b)
    assert len(got) == len(want)


def test_calls_into_the_library_equal_the_recorded_ones():
    compare(record())


def test_every_symbol_the_binding_calls_is_logged_by_its_prototype():
    """The pin reaches the library's entry points through the header alone: every symbol a class of capi.py calls is among its prototypes."""
    called = {line.split()[0] for line in open(FIXTURE) if not line.startswith("#")}
    assert called <= {name for name, _, _ in prototypes()} and len(called) > 70


if __name__ == "__main__":
    args = sys.argv[1:]
    write = "--write" in args
    if write:
        args.remove("--write")
    assert not args or args[0] == "--capi" and len(args) == 2, __doc__
    path = os.path.abspath(args[1]) if args else CAPI
    got = record(path)
    if write:
        with open(FIXTURE, "w") as f:
            f.write(got)
        print("%s: %d lines" % (FIXTURE, len(got.splitlines())))
    else:
        compare(got)
        print("%s reproduced byte for byte by %s" % (os.path.relpath(FIXTURE, ROOT), os.path.relpath(path, ROOT) if path.startswith(ROOT) else path))
