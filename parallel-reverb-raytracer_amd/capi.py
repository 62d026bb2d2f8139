"""ctypes binding of include/rvb_capi.h (librvb_hip.so) for tests and bench.py.

The method names follow the reference's host API for the path (reference rayverb/rayverb.h):
`Raytracer.raytrace / getRawDiffuse / getRawImages / getAllRaw`, `SpeakerAttenuator.attenuate`,
`HrtfAttenuator.attenuate`, `flattenImpulses`.  There is no CPU fallback: if the shared library is
missing or no gfx950 device is usable this module raises.
"""
import collections
import ctypes
import os

import numpy as np

from .dtypes import ATTENUATED, IMPULSE, NUM_BANDS, SPEAKER, SURFACE, aligned_zeros

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RVB_LIB", os.path.join(_HERE, "librvb_hip.so"))   # RVB_LIB: A/B builds of the same ABI

IMAGE_CANDIDATE = np.dtype([("ray", "<u8"), ("slot", "<u4"), ("index", "<u4"), ("impulse", IMPULSE)])

# The header's macros and enumerators under their names without RVB_; tests/test_capi_host.py holds them, the structures below and
# the signature table against a C program compiled with the header.
OK, ERR_INVALID, ERR_NO_DEVICE, ERR_HIP, ERR_STATE, ERR_CAPACITY = range(6)
IR_DIFFUSE, IR_IMAGES, IR_ALL = 1, 2, 3
IR_FAST, IR_EXACT = 0, 1
PIPELINE_MAX_PAIRS = 8
MAX_SPEAKERS = 64
DECAY_TILE = 4096
DECAY_NORMALISED = 1
DECAY_EDT, DECAY_T20, DECAY_T30, DECAY_C50, DECAY_C80, DECAY_D50, DECAY_TS = range(7)
DECAY_NPARAMS = 7
GRAD_MAP_TILE = 1024
LIVE_TILE = 1024
KEEP_MATERIALS, KEEP_LISTENER = 1, 2
MULTI_REHEARSE_RCCL = 1
TABLE_FLOATS = 360 * 180 * NUM_BANDS     # one ear of the HRTF table; a source table

_vp = ctypes.c_void_p
_u64 = ctypes.c_uint64
_i, _u, _u32, _f, _s = ctypes.c_int, ctypes.c_uint, ctypes.c_uint32, ctypes.c_float, ctypes.c_char_p

# Every entry point of include/rvb_capi.h, in the header's order: (restype, argtypes...).  Every pointer is a c_void_p, which takes None,
# byref(...), a ctypes array, a c_void_p and a raw address, but neither a bare Structure nor a value that is not an address.
_SIGNATURES = {
    "rvb_create": (_i, _vp, _i, _u),
    "rvb_destroy": (None, _vp),
    "rvb_last_error": (_s, _vp),
    "rvb_synchronize": (_i, _vp),
    "rvb_wait_for_event": (_i, _vp, _vp),
    "rvb_record_event": (_i, _vp, _vp),
    "rvb_device_info": (_i, _vp, _vp, _u64, _vp, _vp),
    "rvb_device_index": (_i, _vp, _vp),
    "rvb_set_scene": (_i, _vp, _vp, _u64, _vp, _u64, _vp, _u64),
    "rvb_share_scene": (_i, _vp, _vp),
    "rvb_scene_info": (_i, _vp, _vp, _vp, _vp),
    "rvb_set_directions": (_i, _vp, _vp, _u64),
    "rvb_set_directions_device": (_i, _vp, _vp, _u64),
    "rvb_set_concurrent_traces": (_i, _vp, _u32),
    "rvb_set_path_lanes": (_i, _vp, _u32),
    "rvb_trace": (_i, _vp, _vp, _vp, _u64, _vp, _u64),
    "rvb_trace_pairs": (_i, _vp, _vp, _vp, _u64, _u64, _vp, _u64),
    "rvb_trace_group": (_i, _vp, _u64, _vp, _vp, _u64, _vp, _vp),
    "rvb_set_source_pattern": (_i, _vp, _vp, _u64),
    "rvb_set_source_table": (_i, _vp, _vp, _vp, _u64),
    "rvb_keep_paths": (_i, _vp, _i),
    "rvb_reshade": (_i, _vp, _vp, _u64, _vp),
    "rvb_relisten": (_i, _vp, _vp, _u64),
    "rvb_reshade_grad": (_i, _vp, _f, _f, _u64, _vp, _vp, _vp),
    "rvb_reshade_grad_map": (_i, _vp, _f, _f, _u64, _vp, _vp, _u64),
    "rvb_decay_curve": (_i, _vp, _vp, _u64, _u64, _vp),
    "rvb_decay_times": (_i, _vp, _vp, _u64, _u64, _f, _f, _f, _vp),
    "rvb_decay_loss": (_i, _vp, _vp, _vp, _vp, _vp, _u64, _u64, _u, _vp, _vp),
    "rvb_decay_params": (_i, _vp, _vp, _u64, _u64, _f, _vp),
    "rvb_decay_params_loss": (_i, _vp, _vp, _vp, _u64, _u64, _f, _vp, _vp, _vp, _vp, _vp),
    "rvb_ir_select_pair": (_i, _vp, _u64),
    "rvb_get_diffuse": (_i, _vp, _vp),
    "rvb_diffuse_device": (_i, _vp, _vp, _vp),
    "rvb_get_direct": (_i, _vp, _vp),
    "rvb_get_image_candidates": (_i, _vp, _vp, _u64, _vp),
    "rvb_merge_images": (_i, _vp, _u64, _vp, _i, _vp, _u64, _vp),
    "rvb_attenuate_speaker": (_i, _vp, _vp, _vp, _u64, _vp, _vp),
    "rvb_attenuate_speaker_device": (_i, _vp, _vp, _vp, _u64, _vp, _vp),
    "rvb_attenuate_hrtf": (_i, _vp, _vp, _vp, _u64, _vp, _vp, _vp, _u64, _vp),
    "rvb_attenuate_hrtf_device": (_i, _vp, _vp, _vp, _u64, _vp, _vp, _vp, _u64, _vp),
    "rvb_flatten": (_i, _vp, _vp, _u64, _f, _vp, _u64, _vp),
    "rvb_ir_configure_speakers": (_i, _vp, _vp, _vp, _u64, _i, _vp, _u64),
    "rvb_ir_configure_hrtf": (_i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _u64),
    "rvb_ir_time_range": (_i, _vp, _vp, _vp),
    "rvb_ir_time_range_begin": (_i, _vp),
    "rvb_ir_bins": (_u64, _f, _f, _f),
    "rvb_ir_accumulate": (_i, _vp, _f, _f, _u64, _i, _vp),
    "rvb_ir_accumulate_export": (_i, _vp, _f, _f, _u64, _i, _vp, _vp, _u32),
    "rvb_ir_exact_prepare": (_i, _vp, _f, _f, _u64),
    "rvb_ir_exact_fold": (_i, _vp, _u64, _u64, _u64, _vp),
    "rvb_ir_download": (_i, _vp, _i, _f, _i, _vp, _u64, _vp),
    "rvb_device_alloc": (_i, _vp, _u64, _vp),
    "rvb_device_free": (_i, _vp, _vp),
    "rvb_copy_to_host": (_i, _vp, _vp, _vp, _u64),
    "rvb_copy_to_device": (_i, _vp, _vp, _vp, _u64),
    "rvb_host_alloc": (_i, _vp, _u64, _vp),
    "rvb_host_free": (_i, _vp, _vp),
    "rvb_copy_to_pinned_host_async": (_i, _vp, _vp, _vp, _u64),
    "rvb_synchronize_exports": (_i, _vp),
    "rvb_fix_predelay_device": (_i, _vp, _vp, _u64, _f),
    "rvb_flatten_device": (_i, _vp, _vp, _u64, _f, _vp, _u64, _vp),
    "rvb_multi_create": (_i, _vp, _vp, _i, _u),
    "rvb_multi_destroy": (None, _vp),
    "rvb_multi_last_error": (_s, _vp),
    "rvb_multi_devices": (_i, _vp),
    "rvb_multi_context": (_i, _vp, _i, _vp, _vp, _vp),
    "rvb_multi_set_chain_blocks": (_i, _vp, _u32),
    "rvb_multi_peer_links": (_i, _vp),
    "rvb_multi_used_rccl": (_i, _vp),
    "rvb_multi_set_scene": (_i, _vp, _vp, _u64, _vp, _u64, _vp, _u64),
    "rvb_multi_set_directions": (_i, _vp, _vp, _u64),
    "rvb_multi_set_source_pattern": (_i, _vp, _vp),
    "rvb_multi_trace": (_i, _vp, _vp, _vp, _u64, _vp),
    "rvb_multi_get_diffuse": (_i, _vp, _vp),
    "rvb_multi_get_images": (_i, _vp, _i, _vp, _u64, _vp),
    "rvb_multi_ir_speakers": (_i, _vp, _vp, _vp, _u64, _i, _i, _i, _f, _i, _vp, _u64, _vp),
    "rvb_multi_ir_hrtf": (_i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _f, _i, _vp, _u64, _vp),
    "rvb_pipeline_create": (_i, _vp, _vp, _u64, _u64),
    "rvb_pipeline_destroy": (None, _vp),
    "rvb_pipeline_last_error": (_s, _vp),
    "rvb_pipeline_configure_speakers": (_i, _vp, _vp, _u64, _i, _i, _i, _f, _i, _u64, _vp),
    "rvb_pipeline_configure_hrtf": (_i, _vp, _vp, _vp, _vp, _i, _i, _i, _f, _i, _u64, _vp),
    "rvb_pipeline_submit": (_i, _vp, _vp, _vp),
    "rvb_pipeline_submit_oriented": (_i, _vp, _vp, _vp, _vp, _vp),
    "rvb_pipeline_set_source_pattern": (_i, _vp, _vp, _vp),
    "rvb_pipeline_submit_directed": (_i, _vp, _vp, _vp, _vp, _vp, _vp),
    "rvb_pipeline_pending": (_u64, _vp),
    "rvb_pipeline_next": (_i, _vp, _vp),
    "rvb_pipeline_create_lanes": (_i, _vp, _vp, _u64, _vp, _u64, _vp),
    "rvb_last_timings": (_i, _vp, _vp, _u64, _vp, _u64, _vp),
    "rvb_debug_stamps": (_i, _vp, _vp, _u64),
    "rvb_executed_bounces": (_i, _vp, _vp),
}
SYMBOLS = list(_SIGNATURES)
# ... and of include/rvb_capi_images.h, the image sources of a kept trace on the device: a table of its own beside the first
# (tests/test_images_header_host.py holds it against that header)
_IMAGE_SIGNATURES = {
    "rvb_ir_configure_speakers_merged": (_i, _vp, _vp, _vp, _u64, _i, _i, _vp),
    "rvb_ir_configure_hrtf_merged": (_i, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp),
    "rvb_reshade_grad_images": (_i, _vp, _f, _f, _u64, _vp, _vp, _vp),
}
IMAGE_SYMBOLS = list(_IMAGE_SIGNATURES)
# ... and of include/rvb_capi_live.h, the diagnostic of exact mode's live list (tests/test_live_header_host.py)
_LIVE_SIGNATURES = {
    "rvb_ir_exact_list_info": (_i, _vp, _vp, _vp, _vp),
}
LIVE_SYMBOLS = list(_LIVE_SIGNATURES)
# ... and of include/rvb_capi_window.h, the echo finder (tests/test_window_header_host.py), with its constants and structures
_WINDOW_SIGNATURES = {
    "rvb_window_select": (_i, _vp, _vp, _u64, _f, _f, _vp, _u64, _vp, _vp, _vp),
    "rvb_window_paths": (_i, _vp, _f, _f, _vp, _u64, _u64, _vp, _vp, _vp, _vp),
}
WINDOW_SYMBOLS = list(_WINDOW_SIGNATURES)
WINDOW_TILE = 1024
WINDOW_MAX_PATHS = 1024
WINDOW_ENTRY = np.dtype([("record", "<u8"), ("score", "<f4"), ("time", "<f4")])
WINDOW_PATH = np.dtype([("ray", "<u8"), ("bounce", "<u4"), ("nhits", "<u4"), ("score", "<f4"), ("time", "<f4"), ("pad_", "<f4", (2,)),
                        ("volume", "<f4", (NUM_BANDS,))])
WINDOW_HIT = np.dtype([("position", "<f4", (3,)), ("triangle", "<u4")])
# ... and of include/rvb_capi_speech.h, modulation transfer and the speech transmission index (tests/test_speech_header_host.py)
_SPEECH_SIGNATURES = {
    "rvb_mtf": (_i, _vp, _vp, _u64, _u64, _f, _vp, _u64, _vp, _vp),
    "rvb_mtf_adjoint": (_i, _vp, _vp, _u64, _u64, _f, _vp, _u64, _vp, _vp),
    "rvb_speech_index": (_i, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp),
}
SPEECH_SYMBOLS = list(_SPEECH_SIGNATURES)
MTF_MAX_FREQS = 16
STI_BANDS = 7
STI_FREQS = 14
# ... and of include/rvb_capi_source_grad.h, the source-end gradients of a kept trace (tests/test_source_grad_header_host.py)
_SOURCE_GRAD_SIGNATURES = {
    "rvb_source_grad": (_i, _vp, _f, _f, _u64, _vp, _vp, _vp, _vp),
    "rvb_source_grad_images": (_i, _vp, _f, _f, _u64, _vp, _vp, _vp, _vp, _vp),
}
SOURCE_GRAD_SYMBOLS = list(_SOURCE_GRAD_SIGNATURES)
_lib = None


class RvbError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("rvb error %d: %s" % (code, message))
        self.code = code


def load_library():
    """Loads librvb_hip.so (built by `make -C parallel-reverb-raytracer_amd`); raises if absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("%s not built: run __graft_entry__.build() (no CPU fallback exists)" % LIB_PATH)
        # torch brings its own copy of the HIP runtime; if this library's copy initialises the GPU first, torch.cuda later reports
        # "No HIP GPUs are available" (two runtimes in one process, load-order dependent).  Let torch go first when it is there:
        # device tensors handed over by pointer (bench.py, distributed.py) need it anyway.
        try:
            import torch
            if torch.cuda.is_available():
                torch.cuda.init()
        except ImportError:
            pass
        lib = ctypes.CDLL(LIB_PATH)
        for table in (_SIGNATURES, _IMAGE_SIGNATURES, _LIVE_SIGNATURES, _WINDOW_SIGNATURES, _SPEECH_SIGNATURES, _SOURCE_GRAD_SIGNATURES):
            for name, (restype, *argtypes) in table.items():
                function = getattr(lib, name)
                function.restype, function.argtypes = restype, argtypes
        _lib = lib
    return _lib


def _f3(v):
    return (ctypes.c_float * 3)(*[float(x) for x in v])


def _f8(v):
    return (ctypes.c_float * 8)(*[float(x) for x in v])


def _ptr(a):
    return a.ctypes.data_as(_vp) if a is not None else None


def _gain_table(table, ears=1):
    t = np.ascontiguousarray(table, dtype=np.float32).reshape(-1)
    assert t.shape[0] == ears * TABLE_FLOATS
    return t


def _images(images):
    return np.ascontiguousarray(images, dtype=IMPULSE) if images is not None else np.zeros(0, dtype=IMPULSE)


def _query_then_fill(check, function, args, allocate, fill_empty=True):
    """The double call of an entry point that ends in (out, capacity, count *): the size query without a buffer, `allocate(count)`, the fill."""
    count = _u64(0)
    check(function(*args, None, 0, ctypes.byref(count)))
    out = allocate(count.value)
    if count.value or fill_empty:
        check(function(*args, _ptr(out), count.value, ctypes.byref(count)))
    return out


def make_speakers(directions, coefficients):
    sp = aligned_zeros(len(coefficients), SPEAKER)
    sp["direction"][:, :3] = np.asarray(directions, np.float32).reshape(-1, 3)
    sp["coefficient"] = np.asarray(coefficients, np.float32)
    return sp


class SourcePattern(ctypes.Structure):
    """rvb_source_pattern of include/rvb_capi.h: the way the source faces, and a polar-pattern shape per band."""
    _fields_ = [("direction", ctypes.c_float * 4), ("shape", ctypes.c_float * 8)]


def _shape8(shape):
    s = np.asarray(shape, dtype=np.float32).reshape(-1)
    if s.shape[0] == 1:
        s = np.repeat(s, 8)
    assert s.shape[0] == 8, "shape: a scalar or eight values"
    return s


def make_source_patterns(directions, shapes):
    """An array of SourcePattern: directions [n][3]; shapes a scalar, eight values (for all patterns) or [n][8]."""
    d = np.asarray(directions, dtype=np.float32).reshape(-1, 3)
    sh = np.asarray(shapes, dtype=np.float32)
    per = sh.reshape(d.shape[0], 8) if sh.size == 8 * d.shape[0] and sh.ndim == 2 else np.tile(_shape8(sh), (d.shape[0], 1))
    out = (SourcePattern * d.shape[0])()
    for i in range(d.shape[0]):
        out[i].direction[:3] = [float(x) for x in d[i]]
        out[i].shape[:] = [float(x) for x in per[i]]
    return out


class SourcePatternGrad(ctypes.Structure):
    """rvb_source_pattern_grad of include/rvb_capi_source_grad.h: dL/dshape per band, and dL/ddirection with the direction taken as a free
    3-vector (direction[3] = 0)."""
    _fields_ = [("shape", ctypes.c_float * 8), ("direction", ctypes.c_float * 4)]


class SourceOrientation(ctypes.Structure):
    """rvb_source_orientation of include/rvb_capi.h: the way the source faces and its up vector, as rvb_ir_configure_hrtf takes them."""
    _fields_ = [("facing", ctypes.c_float * 4), ("up", ctypes.c_float * 4)]


def make_source_orientations(facing, up):
    """An array of SourceOrientation: facing and up [3] or [n][3] (one of them may be [3] for all n)."""
    f = np.asarray(facing, dtype=np.float32).reshape(-1, 3)
    u = np.asarray(up, dtype=np.float32).reshape(-1, 3)
    n = max(f.shape[0], u.shape[0])
    f, u = np.broadcast_to(f, (n, 3)), np.broadcast_to(u, (n, 3))
    out = (SourceOrientation * n)()
    for i in range(n):
        out[i].facing[:3] = [float(x) for x in f[i]]
        out[i].up[:3] = [float(x) for x in u[i]]
    return out


def surface_table(surfaces):
    """The (array, count) that rvb_reshade takes: a contiguous rvb_surface array, or (None, 0) for the scene's own table."""
    if surfaces is None:
        return None, 0
    table = np.ascontiguousarray(surfaces, dtype=SURFACE).reshape(-1)
    return table, int(table.shape[0])


def _merge_check(rc):
    if rc:
        raise RvbError(rc, "rvb_merge_images")


def merge_images(candidates, direct, remove_direct):
    """Host de-dup of image-source candidates (reference rayverb.cpp:654-676 + :692-706)."""
    lib = load_library()
    cand = np.ascontiguousarray(candidates, dtype=IMAGE_CANDIDATE)
    d = np.ascontiguousarray(direct, dtype=IMPULSE) if direct is not None else None
    return _query_then_fill(_merge_check, lib.rvb_merge_images, (_ptr(cand), cand.shape[0], _ptr(d), int(remove_direct)),
                            lambda count: np.zeros(count, dtype=IMPULSE))


def speech_index(mtf, alpha, beta, snr_db=None, want_derivative=False):
    """(sti, mti float64 [7]) or, with want_derivative, (sti, mti, dSTI/dmtf float64 [7][nfreqs]) of a matrix mtf [7][nfreqs] of modulation
    transfer values, band k in row k (rvb_speech_index: host arithmetic in binary64, no context and no GPU).  alpha [7] and beta [6] are
    the band weights and the redundancy weights, snr_db [7] the signal-to-noise ratios in dB (None: noiseless, +inf for a band likewise).
    A NaN in mtf gives a NaN index."""
    mtf = np.ascontiguousarray(mtf, dtype=np.float64)
    assert mtf.ndim == 2 and mtf.shape[0] == STI_BANDS, "mtf: float64 [7][nfreqs]"
    alpha = np.ascontiguousarray(alpha, dtype=np.float64).reshape(STI_BANDS)
    beta = np.ascontiguousarray(beta, dtype=np.float64).reshape(STI_BANDS - 1)
    snr = None if snr_db is None else np.ascontiguousarray(snr_db, dtype=np.float64).reshape(STI_BANDS)
    sti = ctypes.c_double(0.0)
    mti = np.zeros(STI_BANDS, dtype=np.float64)
    derivative = np.zeros(mtf.shape, dtype=np.float64) if want_derivative else None
    rc = load_library().rvb_speech_index(_ptr(mtf), mtf.shape[1], _ptr(snr), _ptr(alpha), _ptr(beta), ctypes.byref(sti), _ptr(mti), _ptr(derivative))
    if rc != OK:
        raise RvbError(rc, "rvb_speech_index: a required array is missing, or nfreqs is 0 or above %d" % MTF_MAX_FREQS)
    return (sti.value, mti, derivative) if want_derivative else (sti.value, mti)


class _Handle:
    """A handle of the library and its owner: the class names the symbols that destroy it and that give its error text."""
    _destroy = _last_error = None

    def _create(self, symbol, *args):
        self.lib = load_library()
        self.handle = _vp()
        rc = getattr(self.lib, symbol)(ctypes.byref(self.handle), *args)
        if rc:
            raise RvbError(rc, self._create_error(symbol))

    def _create_error(self, symbol):
        return self.lib.rvb_last_error(None).decode()

    def close(self):
        if self.handle:
            getattr(self.lib, self._destroy)(self.handle)
            self.handle = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc:
            raise RvbError(rc, getattr(self.lib, self._last_error)(self.handle).decode())


class Context(_Handle):
    """One GPU, one HIP stream (rvb_ctx)."""
    _destroy, _last_error = "rvb_destroy", "rvb_last_error"

    def __init__(self, device=0):
        self._create("rvb_create", device, 0)
        self.nrays = 0
        self.nreflections = 0
        self.npairs = 1
        self.ray_offset = 0
        self.nchannels = 0
        self.nsurfaces = 0
        self.ntriangles = 0
        self.nimages = 0
        self._keep = []
        self._events = collections.deque(maxlen=2)     # the torch events of the last TWO waits, whichever method made them

    def _traced(self, nreflections, npairs, ray_offset):
        self.nreflections = int(nreflections)
        self.npairs = int(npairs)
        self.ray_offset = int(ray_offset)

    # ---- Raytracer ------------------------------------------------------------------------------
    def set_scene(self, scene):
        triangles, vertices, surfaces = scene
        triangles, vertices, surfaces = (np.ascontiguousarray(x) for x in (triangles, vertices, surfaces))
        self._check(self.lib.rvb_set_scene(self.handle, _ptr(triangles), triangles.shape[0], _ptr(vertices), vertices.shape[0],
                                           _ptr(surfaces), surfaces.shape[0]))
        self.nsurfaces = int(surfaces.shape[0])
        self.ntriangles = int(triangles.shape[0])

    def share_scene(self, other):
        """This context reads the scene `other` holds: the same device buffers, no second build or copy (rvb_share_scene)."""
        self._check(self.lib.rvb_share_scene(self.handle, other.handle))
        self.nsurfaces = other.nsurfaces
        self.ntriangles = other.ntriangles

    def scene_info(self):
        nodes, kept, depth = _u64(0), _u64(0), ctypes.c_uint32(0)
        self._check(self.lib.rvb_scene_info(self.handle, ctypes.byref(nodes), ctypes.byref(kept), ctypes.byref(depth)))
        return {"nodes": nodes.value, "kept_triangles": kept.value, "depth": depth.value}

    def device_info(self):
        arch = ctypes.create_string_buffer(64)
        cus, hbm = ctypes.c_int(0), _u64(0)
        self._check(self.lib.rvb_device_info(self.handle, arch, 64, ctypes.byref(cus), ctypes.byref(hbm)))
        return {"arch": arch.value.decode(), "compute_units": cus.value, "hbm_bytes": hbm.value}

    def set_directions(self, directions):
        d = np.ascontiguousarray(np.asarray(directions, np.float32).reshape(-1, 4))
        self._check(self.lib.rvb_set_directions(self.handle, _ptr(d), d.shape[0]))
        self.nrays = d.shape[0]

    def set_directions_device(self, device_pointer, nrays):
        self._check(self.lib.rvb_set_directions_device(self.handle, device_pointer, nrays))
        self.nrays = nrays

    @staticmethod
    def trace_group(contexts, mics, sources, nreflections, air, ray_offsets=None):
        """rvb_trace on several contexts of one device with ONE path-kernel launch (rvb_trace_group)."""
        n = len(contexts)
        handles = (ctypes.c_void_p * n)(*[c.handle for c in contexts])
        m = np.ascontiguousarray(np.asarray(mics, dtype=np.float32).reshape(n, 3))
        s = np.ascontiguousarray(np.asarray(sources, dtype=np.float32).reshape(n, 3))
        offs = (ctypes.c_uint64 * n)(*[int(o) for o in (ray_offsets if ray_offsets is not None else [0] * n)])
        contexts[0]._check(contexts[0].lib.rvb_trace_group(handles, n, _ptr(m), _ptr(s), nreflections, _f8(air), offs))
        for c, offset in zip(contexts, offs):
            c._traced(nreflections, 1, offset)

    def set_concurrent_traces(self, traces):
        """Hint: traces of this size the caller keeps in flight on the device at a time (rvb_set_concurrent_traces)."""
        self._check(self.lib.rvb_set_concurrent_traces(self.handle, int(traces)))

    def set_path_lanes(self, lanes):
        """Test / measurement hook: lanes per ray of this context's path kernel (4, 2, 1; 0 = chosen per launch).  Same bytes either way."""
        self._check(self.lib.rvb_set_path_lanes(self.handle, int(lanes)))

    def set_source_pattern(self, direction, shape=None):
        """Directional source for the traces that follow (rvb_set_source_pattern): the source faces `direction` and radiates with
        `shape` — a scalar or eight values, one per band: 0 omni, 0.5 cardioid, 1 figure-of-eight.  direction None (or shape None)
        switches it off.  `direction` [n][3] with n > 1 is the per-pair form of trace_pairs (shape: scalar, eight values or [n][8])."""
        pats = make_source_patterns(direction, shape) if direction is not None and shape is not None else None
        self._check(self.lib.rvb_set_source_pattern(self.handle, pats, len(pats) if pats is not None else 0))

    def set_source_table(self, table, facing=None, up=None):
        """Tabulated source directivity for the traces and re-shades that follow (rvb_set_source_table): `table` [360][180][8] band gains
        in the layout of one ear of the HRTF table (directivity.py builds one from a function or a balloon), the source facing `facing`
        with `up` up; [n][3] is the per-pair form of trace_pairs.  It replaces a pattern; table None switches it off."""
        if table is None:
            self._check(self.lib.rvb_set_source_table(self.handle, None, None, 0))
            return
        t = _gain_table(table)
        o = make_source_orientations(facing, up)
        self._check(self.lib.rvb_set_source_table(self.handle, _ptr(t), o, len(o)))

    def keep_paths(self, on, listener=False):
        """The traces that follow keep what reshade needs (rvb_keep_paths): 16 bytes per (ray, bounce); False frees them again.
        listener=True: and what relisten needs (RVB_KEEP_LISTENER), 8 bytes more."""
        keep = (KEEP_MATERIALS | (KEEP_LISTENER if listener else 0)) if on else 0
        self._check(self.lib.rvb_keep_paths(self.handle, keep))

    def relisten(self, mics):
        """The results of the last trace (made with keep_paths(True, listener=True)) as if it had been made with the microphone(s) `mics`
        — one (x, y, z), or [npairs][3] after trace_pairs — (rvb_relisten): no path stage, no record grouping."""
        m = np.ascontiguousarray(np.asarray(mics, dtype=np.float32).reshape(-1, 3))
        self._check(self.lib.rvb_relisten(self.handle, _ptr(m), m.shape[0]))

    def reshade(self, surfaces, air):
        """The results of the last trace (made with keep_paths(True)) as if the scene had the surface table `surfaces` — None: the
        scene's own — and the trace the air coefficients `air` (rvb_reshade): no path stage, no shadow rays."""
        table, count = surface_table(surfaces)
        self._check(self.lib.rvb_reshade(self.handle, _ptr(table), count, _f8(air)))

    def reshade_grad(self, predelay, sample_rate, nbins, device_weights_pointer):
        """(grads, grad_air) of L = sum w * H (rvb_reshade_grad): H the histogram ir_accumulate(predelay, sample_rate, nbins, IR_FAST) adds
        for the selected pair's diffuse records under the configured speakers, w a device array of floats [nchannels][8][nbins].  grads is a
        SURFACE array of the scene's length holding dL/dspecular and dL/ddiffuse, grad_air a float32[8]; both at the table and air that the
        records reflect now.  Synchronous."""
        grads = np.zeros(self.nsurfaces, dtype=SURFACE)
        grad_air = np.zeros(8, dtype=np.float32)
        self._check(self.lib.rvb_reshade_grad(self.handle, predelay, sample_rate, nbins, device_weights_pointer, _ptr(grads), _ptr(grad_air)))
        return grads, grad_air

    def reshade_grad_images(self, predelay, sample_rate, nbins, device_weights_pointer):
        """(grads, grad_air) of the IMAGE part of L = sum w * H (rvb_reshade_grad_images of include/rvb_capi_images.h): what
        ir_accumulate(predelay, sample_rate, nbins, IR_FAST) adds for the images of a configuration made with ir_configure_speakers_merged
        (IR_IMAGES or IR_ALL, at most 8 channels).  grads holds dL/dspecular, its diffuse entries are +0; the direct sound adds to grad_air
        alone.  L is a sum over impulses: add reshade_grad's result (under an IR_DIFFUSE configuration) for the whole of IR_ALL.  Synchronous."""
        grads = np.zeros(self.nsurfaces, dtype=SURFACE)
        grad_air = np.zeros(8, dtype=np.float32)
        self._check(self.lib.rvb_reshade_grad_images(self.handle, predelay, sample_rate, nbins, device_weights_pointer, _ptr(grads), _ptr(grad_air)))
        return grads, grad_air

    def _source_grad_outputs(self, n, want_grad, want_rows, want_pattern, extra=None):
        """The torch CUDA tensors of a source-gradient call for n rays or images, and its host pattern structure; None where not asked for."""
        import torch
        grad = torch.empty((n, 8), dtype=torch.float32, device="cuda") if want_grad else None
        rows = torch.empty((n,), dtype=torch.int32, device="cuda") if want_rows else None
        more = torch.empty((n, extra), dtype=torch.float32, device="cuda") if extra else None
        pattern = SourcePatternGrad() if want_pattern else None
        torch.cuda.synchronize()                     # (the allocator may hand out memory that work on torch's stream still reads)
        return grad, rows, more, pattern

    @staticmethod
    def _pattern_grad(pattern):
        return None if pattern is None else {"shape": np.array(pattern.shape[:], dtype=np.float32), "direction": np.array(pattern.direction[:3], dtype=np.float32)}

    def source_grad(self, predelay, sample_rate, nbins, device_weights_pointer, want_grad=True, want_rows=False, want_pattern=False):
        """dL/d(source gain) of L = sum w * H per ray (rvb_source_grad of include/rvb_capi_source_grad.h): L, w and the state exactly as
        reshade_grad takes them.  Returns a dict: "grad" a float32 CUDA tensor [nrays][8] (want_grad), "rows" an int32 CUDA tensor [nrays]
        of source-table rows (want_rows; the records must reflect a table), "pattern" {"shape": float32 [8], "direction": float32 [3]},
        the derivatives with respect to the polar pattern that the records reflect, the direction taken as a free vector (want_pattern).
        Synchronous."""
        grad, rows, _, pattern = self._source_grad_outputs(self.nrays, want_grad, want_rows, want_pattern)
        self._check(self.lib.rvb_source_grad(self.handle, predelay, sample_rate, nbins, device_weights_pointer,
                                             grad.data_ptr() if grad is not None else None, rows.data_ptr() if rows is not None else None,
                                             ctypes.byref(pattern) if pattern is not None else None))
        return {"grad": grad, "rows": rows, "pattern": self._pattern_grad(pattern)}

    def source_grad_images(self, predelay, sample_rate, nbins, device_weights_pointer, nimages=None, want_grad=True, want_depart=False, want_rows=False,
                           want_pattern=False):
        """The same per image of a configuration made with ir_configure_speakers_merged (rvb_source_grad_images), `nimages` its length (None:
        what that call returned):
        "grad" [nimages][8] in the merged list's order, "depart" [nimages][4] the departure unit vectors the gain uses, "rows", "pattern"."""
        grad, rows, depart, pattern = self._source_grad_outputs(int(self.nimages if nimages is None else nimages), want_grad, want_rows, want_pattern, extra=4 if want_depart else None)
        self._check(self.lib.rvb_source_grad_images(self.handle, predelay, sample_rate, nbins, device_weights_pointer,
                                                    grad.data_ptr() if grad is not None else None, depart.data_ptr() if depart is not None else None,
                                                    rows.data_ptr() if rows is not None else None, ctypes.byref(pattern) if pattern is not None else None))
        return {"grad": grad, "depart": depart, "rows": rows, "pattern": self._pattern_grad(pattern)}

    def reshade_grad_map(self, predelay, sample_rate, nbins, device_weights_pointer, out=None):
        """The gradient of reshade_grad per TRIANGLE (rvb_reshade_grad_map): a float32 CUDA tensor [ntriangles][16], row t the derivatives of
        L with respect to a private copy of the coefficients of triangle t's surface — specular 0..7, then diffuse 8..15 —, t the index of
        the triangle in the scene given to set_scene.  Needs a trace kept with keep_paths(True, listener=True).  The tensor is a new one
        unless `out` is given; every entry is written.  The context's stream waits for torch's current stream first, and the call returns
        when the map is complete."""
        import torch
        if out is None:
            out = torch.empty((self.ntriangles, 16), dtype=torch.float32, device="cuda")
        assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (self.ntriangles, 16)
        self.ir_accumulate_wait_for_torch()
        self._check(self.lib.rvb_reshade_grad_map(self.handle, predelay, sample_rate, nbins, device_weights_pointer, out.data_ptr(), self.ntriangles))
        self.synchronize()
        return out

    def trace(self, mic, source, nreflections, air, ray_offset=0):
        self._check(self.lib.rvb_trace(self.handle, _f3(mic), _f3(source), nreflections, _f8(air), ray_offset))
        self._traced(nreflections, 1, ray_offset)

    def trace_pairs(self, mics, sources, nreflections, air, ray_offset=0):
        """Several (source, microphone) pairs in one launch (rvb_trace_pairs): [npairs][3] each; every pair uses the rays set on
        this context.  Raw results are [npairs][nrays][nreflections]; select_pair(p) picks the pair the IR calls work on."""
        m = np.ascontiguousarray(np.asarray(mics, dtype=np.float32).reshape(-1, 3))
        s_ = np.ascontiguousarray(np.asarray(sources, dtype=np.float32).reshape(-1, 3))
        assert m.shape == s_.shape and m.shape[0] >= 1
        self._check(self.lib.rvb_trace_pairs(self.handle, _ptr(m), _ptr(s_), m.shape[0], nreflections, _f8(air), ray_offset))
        self._traced(nreflections, m.shape[0], ray_offset)

    def select_pair(self, pair):
        self._check(self.lib.rvb_ir_select_pair(self.handle, pair))

    def get_pair_candidates(self, pair, candidates=None):
        """Image-source candidates of one pair of a trace_pairs launch, ray numbers relative to the pair (the candidates carry the trace's
        ray_offset: ray = ray_offset + pair * nrays + the ray's number within the pair)."""
        cand = self.get_image_candidates() if candidates is None else candidates
        in_launch = cand["ray"] - np.uint64(self.ray_offset)
        mine = cand[(in_launch // np.uint64(self.nrays)) == np.uint64(pair)].copy()
        mine["ray"] -= np.uint64(self.ray_offset + pair * self.nrays)
        return mine

    def raytrace(self, mic, source, directions, nreflections, air):
        """Raytracer::raytrace (reference rayverb.cpp:538-685)."""
        self.set_directions(directions)
        self.trace(mic, source, nreflections, air)

    def synchronize(self):
        self._check(self.lib.rvb_synchronize(self.handle))

    def get_raw_diffuse(self):
        out = np.zeros(self.npairs * self.nrays * self.nreflections, dtype=IMPULSE)
        self._check(self.lib.rvb_get_diffuse(self.handle, _ptr(out)))
        return out

    def diffuse_device(self):
        p, n = _vp(), _u64(0)
        self._check(self.lib.rvb_diffuse_device(self.handle, ctypes.byref(p), ctypes.byref(n)))
        return p.value, n.value

    def get_direct(self):
        out = np.zeros(1, dtype=IMPULSE)
        self._check(self.lib.rvb_get_direct(self.handle, _ptr(out)))
        return out

    def get_image_candidates(self):
        return _query_then_fill(self._check, self.lib.rvb_get_image_candidates, (self.handle,),
                                lambda count: np.zeros(count, dtype=IMAGE_CANDIDATE), fill_empty=False)

    def get_raw_images(self, remove_direct):
        """Raytracer::getRawImages (reference rayverb.cpp:692-706)."""
        direct = self.get_direct() if self.nrays else None
        return merge_images(self.get_image_candidates(), direct, remove_direct)

    def get_all_raw(self, remove_direct):
        return np.concatenate([self.get_raw_diffuse(), self.get_raw_images(remove_direct)])

    def executed_bounces(self):
        v = _u64(0)
        self._check(self.lib.rvb_executed_bounces(self.handle, ctypes.byref(v)))
        return v.value

    def debug_stamps(self):
        out = (ctypes.c_uint64 * 32)()
        self._check(self.lib.rvb_debug_stamps(self.handle, out, 32))
        return [int(x) for x in out]

    def last_timings(self):
        names = ctypes.create_string_buffer(1024)
        ms = (ctypes.c_float * 32)()
        count = _u64(0)
        self._check(self.lib.rvb_last_timings(self.handle, names, 1024, ms, 32, ctypes.byref(count)))
        keys = names.value.decode().split(";") if count.value else []
        return [(k, float(ms[i])) for i, k in enumerate(keys)]

    # ---- SpeakerAttenuator / HrtfAttenuator (materialised, one channel per call) --------------------
    def attenuate_speaker(self, mic, impulses, direction, coefficient):
        imp = np.ascontiguousarray(impulses, dtype=IMPULSE)
        sp = make_speakers([direction], [coefficient])
        out = np.zeros(imp.shape[0], dtype=ATTENUATED)
        self._check(self.lib.rvb_attenuate_speaker(self.handle, _f3(mic), _ptr(imp), imp.shape[0], _ptr(sp), _ptr(out)))
        return out

    def attenuate_speaker_device(self, mic, d_in, n, direction, coefficient, d_out):
        """The materialised `attenuate` kernel on HBM-resident buffers (device addresses), asynchronous."""
        sp = make_speakers([direction], [coefficient])
        self._check(self.lib.rvb_attenuate_speaker_device(self.handle, _f3(mic), d_in, n, _ptr(sp), d_out))

    def attenuate_hrtf_device(self, mic, d_in, n, table_channel, facing, up, channel, d_out):
        """The materialised `hrtf` kernel on HBM-resident buffers (device addresses), asynchronous."""
        table = _gain_table(table_channel)
        self._check(self.lib.rvb_attenuate_hrtf_device(self.handle, _f3(mic), d_in, n, _ptr(table), _f3(facing), _f3(up), channel, d_out))

    def attenuate_hrtf(self, mic, impulses, table_channel, facing, up, channel):
        imp = np.ascontiguousarray(impulses, dtype=IMPULSE)
        table = _gain_table(table_channel)
        out = np.zeros(imp.shape[0], dtype=ATTENUATED)
        self._check(self.lib.rvb_attenuate_hrtf(self.handle, _f3(mic), _ptr(imp), imp.shape[0], _ptr(table), _f3(facing), _f3(up), channel,
                                                _ptr(out)))
        return out

    def flatten(self, attenuated, sample_rate):
        """flattenImpulses for one channel (reference rayverb.cpp:48-77) -> [8][nbins]."""
        a = np.ascontiguousarray(attenuated, dtype=ATTENUATED)
        return _query_then_fill(self._check, self.lib.rvb_flatten, (self.handle, _ptr(a), a.shape[0], sample_rate),
                                lambda nbins: np.zeros((8, nbins), dtype=np.float32))

    # ---- fused impulse-response stage ------------------------------------------------------------------
    def ir_configure_speakers(self, mic, directions, coefficients, which=IR_ALL, images=None):
        sp = make_speakers(directions, coefficients)
        img = _images(images)
        self._check(self.lib.rvb_ir_configure_speakers(self.handle, _f3(mic), _ptr(sp), sp.shape[0], which, _ptr(img), img.shape[0]))
        self.nchannels = sp.shape[0]

    def ir_configure_hrtf(self, mic, table, facing, up, which=IR_ALL, images=None):
        """table: [2][360][180][8] floats, or None = the table of this context's previous ir_configure_hrtf stays on the device (many
        listeners, one table: the 4 MB go up once)."""
        t = _gain_table(table, ears=2) if table is not None else None
        img = _images(images)
        self._check(self.lib.rvb_ir_configure_hrtf(self.handle, _f3(mic), _ptr(t), _f3(facing), _f3(up), which, _ptr(img), img.shape[0]))
        self.nchannels = 2

    def ir_configure_speakers_merged(self, mic, directions, coefficients, which=IR_ALL, remove_direct=False):
        """ir_configure_speakers with images = get_raw_images(remove_direct) of the selected pair, made on the device
        (rvb_ir_configure_speakers_merged of include/rvb_capi_images.h): which candidate wins each key of the merge is decided once per
        trace or relisten, so after a reshade the call costs one gather kernel.  Returns the number of images."""
        sp = make_speakers(directions, coefficients)
        nimages = _u64(0)
        self._check(self.lib.rvb_ir_configure_speakers_merged(self.handle, _f3(mic), _ptr(sp), sp.shape[0], which, int(remove_direct), ctypes.byref(nimages)))
        self.nchannels = sp.shape[0]
        self.nimages = nimages.value                   # (source_grad_images sizes its outputs by it)
        return nimages.value

    def ir_configure_hrtf_merged(self, mic, table, facing, up, which=IR_ALL, remove_direct=False):
        """ir_configure_hrtf with images = get_raw_images(remove_direct) of the selected pair, made on the device
        (rvb_ir_configure_hrtf_merged); table None as in ir_configure_hrtf.  Returns the number of images."""
        t = _gain_table(table, ears=2) if table is not None else None
        nimages = _u64(0)
        self._check(self.lib.rvb_ir_configure_hrtf_merged(self.handle, _f3(mic), _ptr(t), _f3(facing), _f3(up), which, int(remove_direct), ctypes.byref(nimages)))
        self.nchannels = 2
        return nimages.value

    def ir_time_range(self):
        lo, hi = ctypes.c_float(0), ctypes.c_float(0)
        self._check(self.lib.rvb_ir_time_range(self.handle, ctypes.byref(lo), ctypes.byref(hi)))
        return lo.value, hi.value

    def ir_bins(self, max_time, predelay, sample_rate):
        return int(self.lib.rvb_ir_bins(max_time, predelay, sample_rate))

    def ir_accumulate(self, predelay, sample_rate, nbins, mode, device_histogram_pointer):
        self._check(self.lib.rvb_ir_accumulate(self.handle, predelay, sample_rate, nbins, mode, device_histogram_pointer))

    def ir_accumulate_wait_for_torch(self):
        """The context's stream waits (by an event, not the host) for everything enqueued so far on torch's current stream."""
        import torch
        ready = torch.cuda.Event()
        ready.record()
        self._check(self.lib.rvb_wait_for_event(self.handle, ready.cuda_event))
        # The wait has been enqueued, not executed.  The events of the last two waits stay alive (not one slot per kind of caller); an
        # older one may go, since destroying an event that an enqueued wait names is safe in HIP.
        self._events.append(ready)

    def ir_accumulate_tensor(self, predelay, sample_rate, nbins, mode, tensor):
        """Adds into a zeroed torch CUDA tensor [nchannels][8][nbins] (plumbing for distributed.py).  The tensor was
        filled on torch's current stream: the context's stream waits for that fill through an event, the host does not."""
        assert tensor.is_cuda and tensor.is_contiguous() and tensor.numel() == self.nchannels * 8 * nbins
        self.ir_accumulate_wait_for_torch()
        self.ir_accumulate(predelay, sample_rate, nbins, mode, tensor.data_ptr())

    def ir_accumulate_export_tensor(self, predelay, sample_rate, nbins, mode, tensor, pinned_host_tensor, slices=0):
        """ir_accumulate_tensor + export_tensor_to_host in one call (rvb_ir_accumulate_export): in exact mode with the speaker model
        the histogram leaves for the host bin range by bin range while the later ranges are still being folded."""
        assert tensor.is_cuda and tensor.is_contiguous() and tensor.numel() == self.nchannels * 8 * nbins
        assert pinned_host_tensor.is_pinned() and pinned_host_tensor.is_contiguous()
        assert tensor.numel() * tensor.element_size() == pinned_host_tensor.numel() * pinned_host_tensor.element_size()
        self.ir_accumulate_wait_for_torch()
        self._check(self.lib.rvb_ir_accumulate_export(self.handle, predelay, sample_rate, nbins, mode, tensor.data_ptr(),
                                                      pinned_host_tensor.data_ptr(), int(slices)))

    def ir_exact_prepare(self, predelay, sample_rate, nbins):
        """Exact mode, step 1: keys, sort, run boundaries of this context's impulses (rvb_ir_exact_prepare)."""
        self._check(self.lib.rvb_ir_exact_prepare(self.handle, predelay, sample_rate, nbins))

    def ir_exact_fold_tensor(self, nbins, bin_begin, bin_end, tensor):
        """Exact mode, step 2: bins [bin_begin, bin_end) folded on top of what the torch CUDA tensor [nchannels][8][nbins] holds; the
        context's stream first waits (by an event) for what torch's current stream has done to the tensor."""
        assert tensor.is_cuda and tensor.is_contiguous() and tensor.numel() == self.nchannels * 8 * nbins
        self.ir_accumulate_wait_for_torch()
        self._check(self.lib.rvb_ir_exact_fold(self.handle, nbins, bin_begin, bin_end, tensor.data_ptr()))

    def ir_exact_list_info(self):
        """(listed, live_on_device, count_valid) of the last exact-mode list of this context (rvb_ir_exact_list_info)."""
        listed, live, valid = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_int(0)
        self._check(self.lib.rvb_ir_exact_list_info(self.handle, ctypes.byref(listed), ctypes.byref(live), ctypes.byref(valid)))
        return listed.value, live.value, bool(valid.value)

    # ---- the echo finder (include/rvb_capi_window.h) ---------------------------------------------------------------
    @staticmethod
    def _window_weights(weights):
        return _f8(np.asarray(weights, dtype=np.float32).reshape(8)) if weights is not None else None

    def _device_block(self, nbytes, fill=None):
        """A device block of this context's library for a call's results, as a (pointer, free) pair."""
        p = _vp()
        self._check(self.lib.rvb_device_alloc(self.handle, max(int(nbytes), 16), ctypes.byref(p)))
        if fill is not None:
            self._check(self.lib.rvb_copy_to_device(self.handle, p, _ptr(fill), fill.nbytes))
        return p, lambda: self.lib.rvb_device_free(self.handle, p)

    def window_select(self, impulses, n=None, t_begin=0.0, t_end=float("inf"), weights=None, max_entries=WINDOW_MAX_PATHS):
        """(entries, in_window): the strongest records behind the window [t_begin, t_end) of a device array of `n` impulses
        (rvb_window_select) — a torch CUDA tensor (n defaults to its bytes / 64; the context's stream waits for torch's current stream) or
        a device address.  entries is a WINDOW_ENTRY array of min(in_window, max_entries) rows by descending score, equal scores by
        ascending record number; the score is sum_b (weights[b] * volume[b])^2, weights None = ones.  Synchronous."""
        if hasattr(impulses, "data_ptr"):
            assert impulses.is_cuda and impulses.is_contiguous()
            if n is None:
                n = impulses.numel() * impulses.element_size() // IMPULSE.itemsize
            self.ir_accumulate_wait_for_torch()
            impulses = impulses.data_ptr()
        capacity = min(max(int(max_entries), 0), WINDOW_MAX_PATHS)           # (the library refuses what lies outside; nothing is written then)
        d_entries, free = self._device_block(capacity * WINDOW_ENTRY.itemsize)
        try:
            count, inside = _u64(0), _u64(0)
            self._check(self.lib.rvb_window_select(self.handle, impulses or None, int(n), t_begin, t_end, self._window_weights(weights), int(max_entries),
                                                   d_entries, ctypes.byref(count), ctypes.byref(inside)))
            entries = np.zeros(count.value, dtype=WINDOW_ENTRY)
            if count.value:
                self._check(self.lib.rvb_copy_to_host(self.handle, _ptr(entries), d_entries, entries.nbytes))
        finally:
            free()
        return entries, inside.value

    def window_paths(self, t_begin, t_end, weights=None, max_paths=64, max_hits=0):
        """(paths, hits, in_window): the strongest diffuse paths of the selected pair behind the window [t_begin, t_end), from the records
        as they stand now (rvb_window_paths).  paths is a WINDOW_PATH array of min(in_window, max_paths) rows; hits a WINDOW_HIT array
        [rows][max_hits] whose row e holds the first min(paths[e].nhits, max_hits) hits of path e, the rest zero — or None with max_hits
        0, which needs no kept trace (hits need keep_paths(True, listener=True)).  Synchronous."""
        capacity = min(max(int(max_paths), 0), WINDOW_MAX_PATHS)
        d_paths, free_paths = self._device_block(capacity * WINDOW_PATH.itemsize)
        try:
            zeros = np.zeros((capacity, int(max_hits)), dtype=WINDOW_HIT) if max_hits else None
            d_hits, free_hits = self._device_block(zeros.nbytes, zeros) if max_hits else (None, lambda: None)
            try:
                count, inside = _u64(0), _u64(0)
                self._check(self.lib.rvb_window_paths(self.handle, t_begin, t_end, self._window_weights(weights), int(max_paths), int(max_hits),
                                                      d_paths, d_hits, ctypes.byref(count), ctypes.byref(inside)))
                paths = np.zeros(count.value, dtype=WINDOW_PATH)
                hits = np.zeros((count.value, int(max_hits)), dtype=WINDOW_HIT) if max_hits else None
                if count.value:
                    self._check(self.lib.rvb_copy_to_host(self.handle, _ptr(paths), d_paths, paths.nbytes))
                    if max_hits:
                        self._check(self.lib.rvb_copy_to_host(self.handle, _ptr(hits), d_hits, hits.nbytes))
            finally:
                free_hits()
        finally:
            free_paths()
        return paths, hits, inside.value

    # ---- modulation transfer (include/rvb_capi_speech.h): device arrays of nrows rows of nbins floats, the caller's own -------------
    def mtf(self, device_histogram_pointer, nrows, nbins, sample_rate, mod_freqs, want_sums=False):
        """float64 [nrows][nfreqs]: m(F) = |sum_j H_j^2 exp(-2 pi i F j / fs)| / sum_j H_j^2 of every row at the modulation frequencies
        mod_freqs in Hz (rvb_mtf): binary64 sums in a fixed order, NaN in an all-zero row.  With want_sums (mtf, sums), sums float64
        [nrows][1 + 2 nfreqs] = S, A_0, B_0, A_1, ...  Synchronous."""
        freqs = np.ascontiguousarray(mod_freqs, dtype=np.float64).reshape(-1)
        out = np.zeros((int(nrows), freqs.shape[0]), dtype=np.float64)
        sums = np.zeros((int(nrows), 1 + 2 * freqs.shape[0]), dtype=np.float64) if want_sums else None
        self._check(self.lib.rvb_mtf(self.handle, device_histogram_pointer or None, int(nrows), int(nbins), sample_rate, _ptr(freqs), freqs.shape[0],
                                     _ptr(out), _ptr(sums)))
        return (out, sums) if want_sums else out

    def mtf_adjoint(self, device_histogram_pointer, nrows, nbins, sample_rate, mod_freqs, coeffs, device_weights_pointer):
        """w = dL/dH in H's layout at device_weights_pointer (float32 [nrows][nbins], every entry written) for a loss with coeffs
        [nrows][nfreqs] = dL/dm (rvb_mtf_adjoint): what reshade_grad, reshade_grad_images and reshade_grad_map take.  Synchronous."""
        freqs = np.ascontiguousarray(mod_freqs, dtype=np.float64).reshape(-1)
        coeffs = np.ascontiguousarray(coeffs, dtype=np.float64).reshape(int(nrows), freqs.shape[0])
        self._check(self.lib.rvb_mtf_adjoint(self.handle, device_histogram_pointer or None, int(nrows), int(nbins), sample_rate, _ptr(freqs),
                                             freqs.shape[0], _ptr(coeffs), device_weights_pointer or None))

    def export_tensor_to_host(self, tensor, pinned_host_tensor):
        """Enqueues, behind the binning, the copy of a device tensor (the histogram ir_accumulate_tensor filled) into a PINNED host
        tensor of the same size (rvb_copy_to_pinned_host_async: on the context's export stream); synchronize_exports()
        waits for it, synchronize() does not.  The caller keeps `tensor` alive and untouched until then."""
        assert tensor.is_cuda and tensor.is_contiguous() and pinned_host_tensor.is_pinned() and pinned_host_tensor.is_contiguous()
        assert tensor.numel() * tensor.element_size() == pinned_host_tensor.numel() * pinned_host_tensor.element_size()
        self._check(self.lib.rvb_copy_to_pinned_host_async(self.handle, pinned_host_tensor.data_ptr(), tensor.data_ptr(),
                                                           tensor.numel() * tensor.element_size()))

    def synchronize_exports(self):
        self._check(self.lib.rvb_synchronize_exports(self.handle))

    # ---- decay curves (rvb_decay_*): device arrays of nrows rows of nbins floats, the caller's own ------------------
    def decay_curve(self, device_histogram_pointer, nrows, nbins, device_curve_pointer):
        """E[r][k] = sum_{j >= k} H[r][j]^2 (rvb_decay_curve): binary64 sums in a fixed order, rounded to float once.  Asynchronous on the
        context's stream."""
        self._check(self.lib.rvb_decay_curve(self.handle, device_histogram_pointer, nrows, nbins, device_curve_pointer))

    def decay_times(self, device_curve_pointer, nrows, nbins, sample_rate, db_begin=-5.0, db_end=-35.0):
        """Reverberation time in seconds of every row of a curve (rvb_decay_times), extrapolated to 60 dB from the least-squares line of the
        level between db_begin and db_end (-5, -35: T30; 0, -10: EDT); NaN where it is not available.  float32 [nrows].  Synchronous."""
        seconds = np.zeros(int(nrows), dtype=np.float32)
        self._check(self.lib.rvb_decay_times(self.handle, device_curve_pointer, nrows, nbins, sample_rate, db_begin, db_end, _ptr(seconds)))
        return seconds

    def decay_loss(self, device_histogram_pointer, device_curve_pointer, device_target_pointer, device_mask_pointer, nrows, nbins,
                   flags=DECAY_NORMALISED, device_weights_pointer=None):
        """loss_rows float64 [nrows] = sum_k m d^2 with d the difference of the log curves (rvb_decay_loss; flags: DECAY_NORMALISED or 0); with
        device_weights_pointer the adjoint w = dL/dH goes there in H's layout: what reshade_grad takes.  Synchronous."""
        loss_rows = np.zeros(int(nrows), dtype=np.float64)
        self._check(self.lib.rvb_decay_loss(self.handle, device_histogram_pointer, device_curve_pointer, device_target_pointer, device_mask_pointer,
                                            nrows, nbins, int(flags), _ptr(loss_rows), device_weights_pointer or None))
        return loss_rows

    def decay_params(self, device_curve_pointer, nrows, nbins, sample_rate):
        """float32 [nrows][DECAY_NPARAMS]: EDT, T20, T30 (seconds), C50, C80 (dB), D50, Ts (seconds) of every row of a curve in one sweep
        (rvb_decay_params; columns DECAY_EDT .. DECAY_TS); NaN where a parameter is not available.  Synchronous."""
        params = np.zeros((int(nrows), DECAY_NPARAMS), dtype=np.float32)
        self._check(self.lib.rvb_decay_params(self.handle, device_curve_pointer, nrows, nbins, sample_rate, _ptr(params)))
        return params

    def decay_params_loss(self, device_histogram_pointer, device_curve_pointer, nrows, nbins, sample_rate, targets, param_weights,
                          device_weights_pointer=None):
        """(loss_rows float64 [nrows], params float32 [nrows][DECAY_NPARAMS]): loss_rows = sum_p param_weights (q - targets)^2 over the
        parameters with a weight > 0 and a finite model value q (rvb_decay_params_loss); targets and param_weights are host arrays
        [nrows][DECAY_NPARAMS].  With device_weights_pointer the adjoint w = dL/dH goes there in H's layout: what reshade_grad takes.
        Synchronous."""
        targets = np.ascontiguousarray(targets, dtype=np.float32).reshape(int(nrows), DECAY_NPARAMS)
        param_weights = np.ascontiguousarray(param_weights, dtype=np.float32).reshape(int(nrows), DECAY_NPARAMS)
        loss_rows = np.zeros(int(nrows), dtype=np.float64)
        params = np.zeros((int(nrows), DECAY_NPARAMS), dtype=np.float32)
        self._check(self.lib.rvb_decay_params_loss(self.handle, device_histogram_pointer, device_curve_pointer, nrows, nbins, sample_rate,
                                                   _ptr(targets), _ptr(param_weights), _ptr(loss_rows), _ptr(params), device_weights_pointer or None))
        return loss_rows, params

    @staticmethod
    def _decay_rows(tensor, *others):
        """(nrows, nbins) of a float32 CUDA tensor [..., nbins] whose leading dimensions are the rows; the others have its shape."""
        import torch
        for t in (tensor,) + others:
            assert t.is_cuda and t.is_contiguous() and t.dtype == torch.float32 and t.shape == tensor.shape
        assert tensor.dim() >= 1 and tensor.numel() > 0
        return tensor.numel() // tensor.shape[-1], tensor.shape[-1]

    def decay_curve_tensor(self, histogram, curve=None):
        """decay_curve on torch CUDA tensors [..., nbins] (every leading index is a row): the context's stream waits for torch's current
        stream through an event; returns the curve tensor (a new one unless given).  The caller synchronizes the context before torch
        reads it, as after ir_accumulate_tensor."""
        import torch
        if curve is None:
            curve = torch.empty_like(histogram)
        nrows, nbins = self._decay_rows(histogram, curve)
        self.ir_accumulate_wait_for_torch()
        self.decay_curve(histogram.data_ptr(), nrows, nbins, curve.data_ptr())
        return curve

    def decay_times_tensor(self, curve, sample_rate, db_begin=-5.0, db_end=-35.0):
        """decay_times on a torch CUDA tensor [..., nbins]: float32 of the leading shape."""
        nrows, nbins = self._decay_rows(curve)
        self.ir_accumulate_wait_for_torch()
        return self.decay_times(curve.data_ptr(), nrows, nbins, sample_rate, db_begin, db_end).reshape(tuple(curve.shape[:-1]))

    def decay_loss_tensor(self, histogram, curve, target, mask, flags=DECAY_NORMALISED, weights=None):
        """decay_loss on torch CUDA tensors of one shape [..., nbins]: float64 losses of the leading shape; `weights` (a tensor of the same
        shape, or None) receives dL/dH and is complete when the call returns."""
        others = (curve, target, mask) + ((weights,) if weights is not None else ())
        nrows, nbins = self._decay_rows(histogram, *others)
        self.ir_accumulate_wait_for_torch()
        loss = self.decay_loss(histogram.data_ptr(), curve.data_ptr(), target.data_ptr(), mask.data_ptr(), nrows, nbins, flags,
                               weights.data_ptr() if weights is not None else None)
        return loss.reshape(tuple(histogram.shape[:-1]))

    def decay_params_tensor(self, curve, sample_rate):
        """decay_params on a torch CUDA tensor [..., nbins]: float32 of the leading shape with DECAY_NPARAMS behind it — [nchannels][8][7]
        for a curve [nchannels][8][nbins]."""
        nrows, nbins = self._decay_rows(curve)
        self.ir_accumulate_wait_for_torch()
        return self.decay_params(curve.data_ptr(), nrows, nbins, sample_rate).reshape(tuple(curve.shape[:-1]) + (DECAY_NPARAMS,))

    def decay_params_loss_tensor(self, histogram, curve, sample_rate, targets, param_weights, weights=None):
        """decay_params_loss on torch CUDA tensors of one shape [..., nbins]: (losses float64 of the leading shape, params float32 of the
        leading shape with DECAY_NPARAMS behind it); targets and param_weights are host arrays of the params' shape; `weights` (a tensor of
        the histogram's shape, or None) receives dL/dH and is complete when the call returns."""
        nrows, nbins = self._decay_rows(histogram, curve, *((weights,) if weights is not None else ()))
        self.ir_accumulate_wait_for_torch()
        loss, params = self.decay_params_loss(histogram.data_ptr(), curve.data_ptr(), nrows, nbins, sample_rate, targets, param_weights,
                                              weights.data_ptr() if weights is not None else None)
        lead = tuple(histogram.shape[:-1])
        return loss.reshape(lead), params.reshape(lead + (DECAY_NPARAMS,))

    def ir_download(self, trim_predelay, sample_rate, mode=IR_FAST):
        """attenuate -> fixPredelay -> flattenImpulses (reference cmd/main.cpp:280-298) -> [nch][8][nbins]."""
        return _query_then_fill(self._check, self.lib.rvb_ir_download, (self.handle, int(trim_predelay), sample_rate, mode),
                                lambda nbins: np.zeros((self.nchannels, 8, nbins), dtype=np.float32))


class MultiContext(_Handle):
    """Several GPUs of one node behind the C-ABI (rvb_multi_*): ray shards, merged image sources, histograms combined on the
    devices (exact mode: one chained serial sum, bit-identical to a single context; fast mode: RCCL all-reduce)."""
    _destroy, _last_error = "rvb_multi_destroy", "rvb_multi_last_error"

    def __init__(self, devices, flags=0):
        devs = (ctypes.c_int * len(devices))(*[int(d) for d in devices])
        self._create("rvb_multi_create", devs, len(devices), flags)
        self.nrays = self.nreflections = 0

    def set_scene(self, scene):
        triangles, vertices, surfaces = (np.ascontiguousarray(x) for x in scene)
        self._check(self.lib.rvb_multi_set_scene(self.handle, _ptr(triangles), triangles.shape[0], _ptr(vertices), vertices.shape[0],
                                                 _ptr(surfaces), surfaces.shape[0]))

    def raytrace(self, mic, source, directions, nreflections, air):
        d = np.ascontiguousarray(np.asarray(directions, np.float32).reshape(-1, 4))
        self._check(self.lib.rvb_multi_set_directions(self.handle, _ptr(d), d.shape[0]))
        self._check(self.lib.rvb_multi_trace(self.handle, _f3(mic), _f3(source), nreflections, _f8(air)))
        self.nrays, self.nreflections = d.shape[0], int(nreflections)

    def set_source_pattern(self, direction, shape=None):
        """Context.set_source_pattern on every device's context (rvb_multi_set_source_pattern); None switches it off."""
        pats = make_source_patterns([direction], shape) if direction is not None and shape is not None else None
        self._check(self.lib.rvb_multi_set_source_pattern(self.handle, pats))

    def shard(self, index):
        first, count = _u64(0), _u64(0)
        self._check(self.lib.rvb_multi_context(self.handle, index, None, ctypes.byref(first), ctypes.byref(count)))
        return first.value, count.value

    def used_rccl(self):
        return bool(self.lib.rvb_multi_used_rccl(self.handle))

    def set_chain_blocks(self, blocks):
        """Bin-range blocks the exact mode's histogram travels in from device to device (rvb_multi_set_chain_blocks; same bytes for any count)."""
        self._check(self.lib.rvb_multi_set_chain_blocks(self.handle, int(blocks)))

    def peer_links(self):
        return int(self.lib.rvb_multi_peer_links(self.handle))

    def get_raw_diffuse(self):
        out = np.zeros(self.nrays * self.nreflections, dtype=IMPULSE)
        self._check(self.lib.rvb_multi_get_diffuse(self.handle, _ptr(out)))
        return out

    def get_raw_images(self, remove_direct):
        return _query_then_fill(self._check, self.lib.rvb_multi_get_images, (self.handle, int(remove_direct)),
                                lambda count: np.zeros(count, dtype=IMPULSE))

    def ir_speakers(self, mic, directions, coefficients, trim_predelay, sample_rate, mode, which=IR_ALL, remove_direct=False):
        sp = make_speakers(directions, coefficients)
        args = (self.handle, _f3(mic), _ptr(sp), sp.shape[0], which, int(remove_direct), int(trim_predelay), sample_rate, mode)
        return _query_then_fill(self._check, self.lib.rvb_multi_ir_speakers, args, lambda nbins: np.zeros((sp.shape[0], 8, nbins), dtype=np.float32))

    def ir_hrtf(self, mic, table, facing, up, trim_predelay, sample_rate, mode, which=IR_ALL, remove_direct=False):
        t = _gain_table(table, ears=2)
        args = (self.handle, _f3(mic), _ptr(t), _f3(facing), _f3(up), which, int(remove_direct), int(trim_predelay), sample_rate, mode)
        return _query_then_fill(self._check, self.lib.rvb_multi_ir_hrtf, args, lambda nbins: np.zeros((2, 8, nbins), dtype=np.float32))


class PipelineResult(ctypes.Structure):
    """rvb_pipeline_result of include/rvb_capi.h."""
    _fields_ = [("job", ctypes.c_uint64), ("histogram", ctypes.POINTER(ctypes.c_float)), ("nchannels", ctypes.c_uint64), ("nbins", ctypes.c_uint64),
                ("predelay", ctypes.c_float), ("max_time", ctypes.c_float), ("nimages", ctypes.c_uint64)]


class PipelineOptions(ctypes.Structure):
    """rvb_pipeline_options of include/rvb_capi.h."""
    _fields_ = [("group", ctypes.c_uint64), ("pairs_per_launch", ctypes.c_uint64)]


class Pipeline(_Handle):
    """Impulse responses back to back behind the C-ABI (rvb_pipeline_*, csrc/pipeline.hip): the native form of
    distributed.IrPipeline — groups of traces in one path-kernel launch, the next groups' traces enqueued ahead, the binning stages of a
    group enqueued together, histograms exported to a ring of pinned buffers.  `contexts`: capi.Context objects of one GPU with the
    same scene and rays set.

    lanes = [[Context, ...], ...] (rvb_pipeline_create_lanes): that schedule per lane, each lane on one device and driven by a host thread
    of its own; unit u of `pairs_per_launch` consecutive jobs goes to lane u % len(lanes) and is traced by ONE rvb_trace_pairs launch.
    `contexts` is then ignored.  lanes=None with pairs_per_launch=1 is rvb_pipeline_create."""
    _destroy, _last_error = "rvb_pipeline_destroy", "rvb_pipeline_last_error"

    def __init__(self, contexts, group=0, lanes=None, pairs_per_launch=1):
        pairs = int(pairs_per_launch)
        one_lane_of_single_jobs = lanes is None and pairs == 1
        lanes = [list(contexts)] if lanes is None else [list(l) for l in lanes]
        self.contexts = [c for l in lanes for c in l]
        count = len(self.contexts)
        handles = (_vp * count)(*[c.handle for c in self.contexts])
        if one_lane_of_single_jobs:
            self._create("rvb_pipeline_create", handles, count, int(group))
            self.limit, self.valid_for = 4 * count, count
            return
        sizes = (_u64 * len(lanes))(*[len(l) for l in lanes])
        opts = PipelineOptions(int(group), pairs)
        self._create("rvb_pipeline_create_lanes", handles, count, sizes, len(lanes), ctypes.byref(opts))
        # pending limit and how many further results a histogram view outlives (include/rvb_capi.h)
        self.limit, self.valid_for = 2 * count * pairs, count * pairs

    def _create_error(self, symbol):
        return symbol + " failed"

    def configure_speakers(self, directions, coefficients, nreflections, air, sample_rate=44100.0, trim_predelay=True, mode=IR_EXACT,
                           which=IR_ALL, remove_direct=False):
        sp = make_speakers(directions, coefficients)
        self._check(self.lib.rvb_pipeline_configure_speakers(self.handle, _ptr(sp), sp.shape[0], which, int(remove_direct), int(trim_predelay),
                                                             sample_rate, mode, nreflections, _f8(air)))

    def configure_hrtf(self, table, facing, up, nreflections, air, sample_rate=44100.0, trim_predelay=True, mode=IR_EXACT, which=IR_ALL,
                       remove_direct=False):
        t = _gain_table(table, ears=2)
        self._check(self.lib.rvb_pipeline_configure_hrtf(self.handle, _ptr(t), _f3(facing), _f3(up), which, int(remove_direct), int(trim_predelay),
                                                         sample_rate, mode, nreflections, _f8(air)))

    def set_source_pattern(self, direction, shape=None):
        """Directional sources for the jobs that follow (rvb_pipeline_set_source_pattern; no jobs may be pending): `shape` a scalar or
        eight values, `direction` the default facing of the source; None switches it off."""
        if direction is None or shape is None:
            self._check(self.lib.rvb_pipeline_set_source_pattern(self.handle, None, None))
            return
        self._check(self.lib.rvb_pipeline_set_source_pattern(self.handle, _f8(_shape8(shape)), _f3(direction)))

    def submit(self, mic, source, facing=None, up=None, source_direction=None):
        if source_direction is not None:
            self._check(self.lib.rvb_pipeline_submit_directed(self.handle, _f3(mic), _f3(source), _f3(facing) if facing is not None else None,
                                                              _f3(up) if up is not None else None, _f3(source_direction)))
        elif facing is None:
            self._check(self.lib.rvb_pipeline_submit(self.handle, _f3(mic), _f3(source)))
        else:
            self._check(self.lib.rvb_pipeline_submit_oriented(self.handle, _f3(mic), _f3(source), _f3(facing), _f3(up)))

    def pending(self):
        return int(self.lib.rvb_pipeline_pending(self.handle))

    def next(self, copy=True):
        """The oldest pending job: (histogram [nchannels][8][nbins] — a copy, or a view of the pipeline's pinned buffer that stays valid
        until `valid_for` further results have been taken —, info dict)."""
        res = PipelineResult()
        self._check(self.lib.rvb_pipeline_next(self.handle, ctypes.byref(res)))
        view = np.ctypeslib.as_array(res.histogram, shape=(int(res.nchannels), 8, int(res.nbins)))
        info = {"job": int(res.job), "nbins": int(res.nbins), "predelay": float(res.predelay), "max_time": float(res.max_time), "images": int(res.nimages)}
        return (view.copy() if copy else view), info
