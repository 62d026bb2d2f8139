"""TEST INFRASTRUCTURE: an abstract model of one rvb_ctx over its whole life, and seeded walks of calls that hold a context against it.

A context (csrc/ctx.h) keeps grow-only device buffers and a dozen validity flags; include/rvb_capi.h states the rules those flags
implement.  ContextModel restates the RULES — each transition cites the header lines it comes from — and answers, for every operation
of a walk, either the error code the call must return or the bytes it must return.  The bytes come from the CPU oracle through World
(computed once per key and never changed): oracle.raytrace for a trace, for a re-shade (the oracle's trace under the other table and
air) and for a relisten (the oracle's trace with the other microphone), test_gpu_source_pattern.expected_records for a source pattern,
and the chain attenuate -> fix_predelay -> flatten of tests/test_gpu_attenuation_edges.py for the impulse-response stage.

Walk drives a context-like object (capi.Context on the GPU: tests/test_gpu_context_walks.py; the CPU stand-in of
tests/test_context_model_host.py) and the model side by side.  An operation is a tuple of plain values drawn from the menus below, so
a failing walk prints a list that replay() takes as it is.

Never used by the product; no torch.cuda here."""
import collections

import numpy as np

import attenuation_edges as ae
from parallel_reverb_raytracer_amd import capi, scenes
from parallel_reverb_raytracer_amd.dtypes import AIR_COEFFICIENTS, IMPULSE, NUM_IMAGE_SOURCE

from test_gpu_reshade import AIR_B, set_b
from test_gpu_source_pattern import FACING, SHAPES, expected_records, same_records
from test_gpu_speaker_arrays import fast_bound

# ---- the menus ------------------------------------------------------------------------------------------------------------------
SCENES = ("shoebox", "cathedral")              # 12 triangles (4 key bits) / scenes.cathedral(3000), 7 surfaces (12 key bits)
NDIRS = (5, 130, 509)
NREFL = (1, 24, 32, 64, 70)                    # 32 and 64: the 16-bit key runs of the trace; the others its 32-bit keys
OFFSETS = (0, 1000)
PAIRS = ((0, 0), (1, 1), (1, 0))               # (microphone, source) of the three pairs of trace_pairs
TABLES = ("own", "B")                          # "short": B without its last surface, which rvb_reshade refuses
AIRS = ("A", "B")                              # AIR_COEFFICIENTS / AIR_B of tests/test_gpu_reshade.py
LAYOUTS = {"s2": ae.EDGE_SPEAKERS[5:7], "s9": ae.EDGE_SPEAKERS, "s9r": ae.EDGE_SPEAKERS[::-1]}
HRTF_TABLES = ("T", "U", None)                 # U: T with its ears exchanged; None: the table that is on the device
IMAGES = ("all", "first3", "none", "e40a", "e40b")
WHICH = (capi.IR_DIFFUSE, capi.IR_IMAGES, capi.IR_ALL)
RATES = (44100.0, 8192.0)
PREDELAYS = ("zero", "min", "above")
NBINS = ("full", "full-1", "one", "p-2", "p-1", "p", "p+1")
FLAT_ARRAYS = ("big", "tiny", "edge")          # 509 x 70 attenuated records, their first five (another array), the time edges
ATT_ARRAYS = ("edge", "bnd")
MAX_RECORDS = len(PAIRS) * max(NDIRS) * max(NREFL)
MAX_CHANNELS = 9

Rec = collections.namedtuple("Rec", "scene table air mics sources ndirs nrefl offset pattern")
Cfg = collections.namedtuple("Cfg", "kind layout which images pair")          # kind: "speakers" / "hrtf"; layout: of LAYOUTS / "T", "U"


def time_bins(time, sample_rate):
    """round(time * sample_rate) of rayverb.cpp:69: half away from zero (time >= 0; x - floor(x) is exact)."""
    x = time * np.float32(sample_rate)
    f = np.floor(x)
    return np.where(x - f >= np.float32(0.5), f + 1, f).astype(np.int64)


def ir_bins(max_time, predelay, sample_rate):
    """rvb_ir_bins (rayverb.h:89, rayverb.cpp:57) in binary32."""
    t = np.float32(max_time) - np.float32(predelay) if max_time > predelay else np.float32(0)
    return int(time_bins(np.array([t], np.float32), sample_rate)[0]) + 1


def serial_add(hist, bins, volume):
    """hist[8][nbins] += every impulse, bin by bin in impulse order in binary32: the reference's serial sum (rayverb.cpp:67-74) continued
    from what the histogram holds.  np.cumsum adds one after the other, so a bin's run is one cumsum behind the bin's value."""
    order = np.argsort(bins, kind="stable")
    b, v = bins[order], volume[order]
    starts = np.r_[0, np.flatnonzero(np.diff(b)) + 1] if b.size else np.zeros(0, np.int64)
    ends = np.r_[starts[1:], b.size]
    for s, e in zip(starts, ends):
        run = np.concatenate([hist[:, b[s]][None, :], v[s:e]]).astype(np.float32)
        hist[:, b[s]] = np.cumsum(run, axis=0, dtype=np.float32)[-1]


class World:
    """Everything a walk can ask for, from the CPU oracle, cached per key."""

    def __init__(self, oracle):
        self.oracle = oracle
        box = scenes.shoebox()
        hall, info = scenes.cathedral(3000)
        f3 = lambda v: tuple(float(x) for x in v)
        self.scenes = {
            "shoebox": {"scene": box, "mics": [(0.5, 1.0, 2.0), (-1.0, -2.0, -20.0)], "sources": [(-0.7, -1.2, -5.0), (1.2, 2.0, 30.0)],
                        "B": set_b(box[2], 1, 1, 0)},
            "cathedral": {"scene": hall, "mics": [f3(info["mic"]), (-10.28, 3.85, -2.24)], "sources": [f3(info["source"]), (-12.0, 2.5, 3.0)],
                          "B": set_b(hall[2], 2, 4, 5)},
        }
        self.dirs = {n: scenes.sphere_directions(n, seed=23) for n in NDIRS}
        table = np.ascontiguousarray(scenes.hrtf_synthetic_table(), dtype=np.float32).reshape(2, 360, 180, 8)
        self.hrtf = {"T": table, "U": np.ascontiguousarray(table[::-1])}
        self.facing, self.up = ae.OBLIQUE["facing"], ae.OBLIQUE["up"]
        edge = ae.time_edge_records(44100.0, (1.0, 1.5, -2.0))[0]
        self.image_lists = {"e40a": edge[:40].copy(), "e40b": edge[40:80].copy(), "none": np.zeros(0, IMPULSE)}
        self.att_arrays = {"edge": ae.speaker_edge_records((1.0, 1.5, -2.0))[0], "bnd": ae.boundary_set(ae.OBLIQUE)[0][:300].copy()}
        self._traces, self._channels, self._flat = {}, {}, None
        self.oracle_traces = 0

    # ---- scenes, tables, air -----------------------------------------------------------------------------------------------------
    def scene(self, name):
        return self.scenes[name]["scene"]

    def table(self, scene, name):
        s = self.scenes[scene]
        return {"own": s["scene"][2], "B": s["B"], "short": s["B"][:-1]}[name]

    @staticmethod
    def air(name):
        return {"A": AIR_COEFFICIENTS, "B": AIR_B}[name]

    def mic(self, scene, index):
        return self.scenes[scene]["mics"][index]

    def source(self, scene, index):
        return self.scenes[scene]["sources"][index]

    # ---- records -----------------------------------------------------------------------------------------------------------------
    def trace(self, scene, table, air, mic, source, ndirs, nrefl, pattern):
        """One pair's records: diffuse, the direct slot, the candidates (ray numbers within the pair), the merged images."""
        key = (scene, table, air, mic, source, ndirs, nrefl, pattern)
        if key not in self._traces:
            geo, dirs, xyz = self.scene(scene), self.dirs[ndirs], self.mic(scene, mic)
            if pattern:
                plain = self.trace(scene, table, air, mic, source, ndirs, nrefl, False)
                diffuse, image, index = plain["diffuse"], plain["image"], plain["index"]
            else:
                self.oracle_traces += 1
                diffuse, image, index = self.oracle.raytrace((geo[0], geo[1], self.table(scene, table)), xyz, self.source(scene, source), dirs, nrefl,
                                                             self.air(air))
            idx = index.reshape(ndirs, NUM_IMAGE_SOURCE)
            rays, slots = np.nonzero(idx[:, 1:])
            flat = rays * NUM_IMAGE_SOURCE + slots + 1
            if pattern:
                case = {"nrefl": nrefl, "dirs": dirs, "diffuse": diffuse, "mic": xyz, "images": np.concatenate([image[:1], image[flat]])}
                diffuse, scaled, _, _ = expected_records(self.oracle, case, FACING, SHAPES)
                image = image.copy()
                image[0], image[flat] = scaled[0], scaled[1:]
            cand = np.zeros(rays.shape[0], capi.IMAGE_CANDIDATE)
            cand["ray"], cand["slot"], cand["index"], cand["impulse"] = rays, slots + 1, idx[rays, slots + 1], image[flat]
            self._traces[key] = {"diffuse": diffuse, "image": image, "index": index, "direct": image[:1].copy(), "cand": cand,
                                 "merged": self.oracle.collect_images(image, index, False)}
        return self._traces[key]

    def pair(self, rec, p):
        return self.trace(rec.scene, rec.table, rec.air, rec.mics[p], rec.sources[p], rec.ndirs, rec.nrefl, rec.pattern)

    def diffuse(self, rec):
        return np.concatenate([self.pair(rec, p)["diffuse"] for p in range(len(rec.mics))])

    def candidates(self, rec):
        parts = []
        for p in range(len(rec.mics)):
            c = self.pair(rec, p)["cand"].copy()
            c["ray"] += np.uint64(rec.offset + p * rec.ndirs)          # include/rvb_capi.h, rvb_trace / rvb_trace_pairs: global ray numbers
            parts.append(c)
        return np.concatenate(parts)

    def images(self, rec, p, name):
        if name in self.image_lists:
            return self.image_lists[name]
        merged = self.pair(rec, p)["merged"]
        return merged if name == "all" else merged[:3]

    # ---- the impulse-response stage ----------------------------------------------------------------------------------------------
    def impulses(self, rec, cfg):
        parts = []
        if cfg.which & capi.IR_DIFFUSE:
            parts.append(self.pair(rec, cfg.pair)["diffuse"])
        if cfg.which & capi.IR_IMAGES:
            parts.append(self.images(rec, cfg.pair, cfg.images))
        return np.concatenate(parts) if parts else np.zeros(0, IMPULSE)

    def channels(self, rec, cfg):
        """The oracle's attenuated channels of the configuration: diffuse records of the pair first, then the images."""
        key = (rec, cfg)
        if key not in self._channels:
            if len(self._channels) > 64:
                self._channels.clear()
            self._channels[key] = self.attenuate_all(self.mic(rec.scene, rec.mics[cfg.pair]), self.impulses(rec, cfg), cfg.kind, cfg.layout)
        return self._channels[key]

    def attenuate_all(self, mic, impulses, kind, layout):
        if kind == "hrtf":
            return [self.oracle.attenuate_hrtf(mic, impulses, self.hrtf[layout][ear], self.facing, self.up, ear) for ear in (0, 1)]
        return [self.oracle.attenuate_speaker(mic, impulses, d, k) for d, k in LAYOUTS[layout]]

    @staticmethod
    def time_range(chans):
        """rvb_ir_time_range: earliest non-zero and latest attenuated time over all channels (0, 0 without any)."""
        t = np.concatenate([c["time"] for c in chans])
        nz = t[t != 0]
        return (float(nz.min()) if nz.size else 0.0), (float(t.max()) if t.size else 0.0)

    def geometry(self, chans, sample_rate, predelay, nbins):
        """(predelay, nbins, the class that nbins is) of the histogram geometry menu."""
        lo, hi = self.time_range(chans)
        if predelay == "zero":
            seconds = 0.0
        elif predelay == "min":
            seconds = lo
        else:                                                    # above the earliest records: an eighth of the distinct times lie below
            times = np.unique(np.concatenate([c["time"] for c in chans]))
            times = times[times != 0]
            seconds = float(times[times.size // 8]) if times.size else 0.0
        full = ir_bins(hi, seconds, sample_rate)
        k = 2
        while (1 << (k + 1)) + 1 < full:
            k += 1
        p = 1 << k
        if nbins in ("p-2", "p-1", "p", "p+1") and p + 1 < full:
            return seconds, p + int(nbins[1:] or 0), nbins
        if nbins == "full-1" and full > 1:
            return seconds, full - 1, nbins
        if nbins == "one":
            return seconds, 1, nbins
        return seconds, full, "full"

    def fixed(self, chans, predelay, sample_rate, nbins):
        """fix_predelay on copies, then without the records whose bin is >= nbins (include/rvb_capi.h, rvb_reshade_grad: "records whose
        bin is >= nbins are skipped"; bin_keys_kernel and histogram_fast_kernel do the same)."""
        out = []
        for c in chans:
            c = c.copy()
            self.oracle.fix_predelay(c, predelay)
            out.append(c[time_bins(c["time"], sample_rate) < nbins])
        return out

    def accumulate(self, hist, chans, predelay, sample_rate, b0=0, b1=None):
        """RVB_IR_EXACT on top of `hist` [nchannels][8][nbins], in place.  On a zeroed histogram, all bins: the oracle chain itself, cut or
        padded to nbins; otherwise the serial sum continued bin by bin."""
        nbins = hist.shape[2]
        b1 = nbins if b1 is None else min(b1, nbins)
        fixed = self.fixed(chans, predelay, sample_rate, nbins)
        if b0 == 0 and b1 == nbins and not hist.view(np.uint32).any():
            for ch, c in enumerate(fixed):
                if c.shape[0]:
                    flat = self.oracle.flatten(c, sample_rate)
                    assert flat.shape[1] <= nbins
                    hist[ch][:, :flat.shape[1]] = flat
            return fixed
        for ch, c in enumerate(fixed):
            bins = time_bins(c["time"], sample_rate)
            inside = (bins >= b0) & (bins < b1)
            serial_add(hist[ch], bins[inside], c["volume"][inside])
        return fixed

    # ---- the materialised calls --------------------------------------------------------------------------------------------------
    def flat_array(self, name):
        if self._flat is None:
            rec = Rec("cathedral", "own", "A", (0,), (0,), 509, 70, 0, False)
            d, k = ae.EDGE_SPEAKERS[5]
            big = self.oracle.attenuate_speaker(self.mic("cathedral", 0), self.pair(rec, 0)["diffuse"], d, k)
            edge = self.oracle.attenuate_speaker((1.0, 1.5, -2.0), ae.time_edge_records(8192.0, (1.0, 1.5, -2.0))[0], d, k)
            self._flat = {"big": np.ascontiguousarray(big), "tiny": big[:5].copy(), "edge": np.ascontiguousarray(edge)}
        return self._flat[name]

    def flatten(self, name, sample_rate):
        return self.oracle.flatten(self.flat_array(name), sample_rate)

    def attenuate(self, array, how):
        """how: a speaker of EDGE_SPEAKERS by number, or ("ear", e) with table T"""
        rec, mic = self.att_arrays[array], ae.OBLIQUE["mic"]
        if isinstance(how, int):
            d, k = ae.EDGE_SPEAKERS[how]
            return self.oracle.attenuate_speaker(mic, rec, d, k)
        return self.oracle.attenuate_hrtf(mic, rec, self.hrtf["T"][how[1]], self.facing, self.up, how[1])


OK, INVALID, STATE = capi.OK, capi.ERR_INVALID, capi.ERR_STATE


class ContextModel:
    """The abstract state of one context and the rules of include/rvb_capi.h that change it.  apply(op) returns (code, want, call):
    the code the call must return, the bytes it must return (None: nothing to compare) and the concrete arguments of the call."""

    def __init__(self, world):
        self.w = world
        self.scene = None              # name of the scene set
        self.ndirs = None              # rays set
        self.rec = None                # Rec: what the records reflect; None: nothing traced (or voided)
        self.pattern = False           # rvb_set_source_pattern: what the NEXT trace or re-shade applies
        self.keep = 0                  # rvb_keep_paths: what the next trace keeps
        self.kept = 0                  # what the last trace kept (0: nothing a re-shade or relisten can use)
        self.pair = 0
        self.cfg = None                # Cfg, or None: no IR configuration
        self.nch = 0                   # channels of the last successful configure (sizes the histogram of a refused call)
        self.hrtf_table = None         # "T" / "U": a two-ear table is on the device; "one": one ear's; None
        self.prepared = None           # (Cfg, Rec, predelay, sample_rate, nbins) of rvb_ir_exact_prepare
        self.prepared_nbins = 16       # nbins of the last prepare, also after it was voided (the nbins a fold passes)
        self.hist = None               # expected histogram [nch][8][nbins]; the walk keeps the device's next to it
        self.geometry = (0.0, 44100.0, 16)
        self.hist_geometry = None      # (nch, predelay, rate, nbins) of the histogram the last accumulate left

    # ---- shared transitions --------------------------------------------------------------------------------------------------------
    def _void_trace(self):
        # rvb_capi.h, at rvb_set_directions: "rvb_set_scene, rvb_share_scene and rvb_set_directions* void the last trace and everything
        # made from it": fetches, select_pair, configure -> STATE; the IR configuration, a prepared list and a kept trace are void
        self.rec, self.cfg, self.prepared, self.kept = None, None, None, 0

    def _new_results(self):
        # rvb_capi.h, rvb_reshade / rvb_relisten: "like a trace it voids the IR configuration and a prepared exact list
        # (rvb_ir_configure_* again; rvb_ir_select_pair is back at 0)"
        self.cfg, self.prepared, self.pair = None, None, 0

    def chans(self):
        return self.w.channels(self.rec, self.cfg)

    def apply(self, op):
        return getattr(self, "op_" + op[0])(*op[1:])

    # ---- scene, rays, settings -----------------------------------------------------------------------------------------------------
    def op_set_scene(self, name):
        self.scene = name
        self._void_trace()
        return OK, None, {"scene": self.w.scene(name)}

    def op_set_directions(self, n):
        self.ndirs = n
        self._void_trace()
        return OK, None, {"dirs": self.w.dirs[n]}

    def op_keep_paths(self, keep):
        # rvb_capi.h, rvb_keep_paths: the buffers come with the next trace; 0 frees them "and rvb_reshade fails until the next kept trace"
        self.keep = keep
        if keep == 0:
            self.kept = 0
        return OK, None, {}

    def op_set_source_pattern(self, on):
        # rvb_capi.h, rvb_set_source_pattern: "for every pair of the traces that follow"; rvb_reshade "applies what is set now"
        self.pattern = bool(on)
        return OK, None, {}

    # ---- traces ------------------------------------------------------------------------------------------------------------------------
    def _trace(self, mics, sources, nrefl, air, offset):
        scene = self.scene or "shoebox"
        call = {"mics": [self.w.mic(scene, m) for m in mics], "sources": [self.w.source(scene, s) for s in sources], "air": self.w.air(air)}
        # rvb_capi.h, RVB_ERR_STATE: "call order (e.g. trace before set_scene)"; a trace needs directions as well
        if self.scene is None or self.ndirs is None:
            return STATE, None, call
        self.rec = Rec(self.scene, "own", air, tuple(mics), tuple(sources), self.ndirs, nrefl, offset, self.pattern)
        self.kept = self.keep              # rvb_keep_paths: "from now on the traces of this context keep what rvb_reshade needs"
        self._new_results()                # rvb_ir_select_pair: "pair 0 after a trace"; the exact list: "rvb_trace ... voids it"
        return OK, None, call

    def op_trace(self, mic, source, nrefl, air, offset):
        return self._trace((mic,), (source,), nrefl, air, offset)

    def op_trace_pairs(self, nrefl, air, offset):
        return self._trace([m for m, _ in PAIRS], [s for _, s in PAIRS], nrefl, air, offset)

    def op_select_pair(self, pair):
        # rvb_capi.h, rvb_ir_select_pair: STATE nothing traced, INVALID no such pair; a successful call voids configuration and list
        if self.rec is None:
            return STATE, None, {}
        if pair >= len(self.rec.mics):
            return INVALID, None, {}
        self.pair, self.cfg, self.prepared = pair, None, None
        return OK, None, {}

    def op_reshade(self, table, air):
        scene = self.scene or "shoebox"
        call = {"surfaces": None if table == "own" else self.w.table(scene, table), "air": self.w.air(air)}
        # rvb_capi.h, rvb_reshade: "RVB_ERR_STATE: nothing traced, the last trace was made without keeping, or rvb_set_scene /
        # rvb_share_scene / rvb_set_directions* came since"; "otherwise nsurfaces must equal the scene's (RVB_ERR_INVALID)";
        # "A failed call leaves the results as they were"
        if self.rec is None or not self.kept:
            return STATE, None, call
        if table == "short":
            return INVALID, None, call
        # "the state that rvb_trace / rvb_trace_pairs would have left with the same microphones, sources, directions, nreflections and
        # ray_offset on a scene whose surface table is `surfaces` and with `air_coefficient`"; "with a source pattern set ... scaled"
        self.rec = self.rec._replace(table=table, air=air, pattern=self.pattern)
        self._new_results()
        return OK, None, call

    def op_relisten(self, extra):
        """every microphone exchanged for the scene's other one; extra: one microphone too many (refused)"""
        scene = self.scene or "shoebox"
        mics = tuple(1 - m for m in self.rec.mics) if self.rec is not None else (0,)
        call = {"mics": [self.w.mic(scene, m) for m in mics] + ([self.w.mic(scene, 0)] if extra else [])}
        # rvb_capi.h, rvb_relisten: STATE "nothing traced, the last trace made without RVB_KEEP_LISTENER, or rvb_set_scene / ... since";
        # INVALID "npairs other than the kept trace's"; "A failed call leaves the results as they were"
        if self.rec is None or not self.kept & capi.KEEP_LISTENER:
            return STATE, None, call
        if extra:
            return INVALID, None, call
        # "the new microphone(s), the same sources, ... and the surface table, air and source patterns that the records reflect now"
        self.rec = self.rec._replace(mics=mics)
        self._new_results()
        return OK, None, call

    # ---- fetches ---------------------------------------------------------------------------------------------------------------------
    def op_get_raw_diffuse(self):
        if self.rec is None:
            return STATE, None, {}
        return OK, self.w.diffuse(self.rec), {}

    def op_get_direct(self):
        # rvb_capi.h, rvb_ir_select_pair: "the pair that rvb_get_direct and the rvb_ir_* calls below work on"
        if self.rec is None:
            return STATE, None, {}
        return OK, self.w.pair(self.rec, self.pair)["direct"], {}

    def op_get_image_candidates(self):
        if self.rec is None:
            return STATE, None, {}
        return OK, self.w.candidates(self.rec), {}

    # ---- the impulse-response stage --------------------------------------------------------------------------------------------------
    def _configure(self, kind, layout, which, images):
        scene = self.scene or "shoebox"
        rec = self.rec if self.rec is not None else Rec(scene, "own", "A", (0,), (0,), 5, 1, 0, False)
        pair = self.pair if self.rec is not None else 0
        cfg = Cfg(kind, layout, which, images, pair)
        call = {"mic": self.w.mic(rec.scene, rec.mics[pair]), "images": self.w.images(rec, pair, images)}
        # rvb_capi.h, rvb_ir_configure_*: needs a trace (step 1 of the fused stage works on the trace's impulses): STATE without one
        if self.rec is None:
            return STATE, None, call
        # "Every successful rvb_ir_configure_* ... replaces the previous configuration as a whole ... and voids a prepared exact list"
        self.cfg, self.prepared = cfg, None
        self.nch = 2 if kind == "hrtf" else len(LAYOUTS[layout])
        return OK, None, call

    def op_configure_speakers(self, layout, which, images):
        code, want, call = self._configure("speakers", layout, which, images)
        call["speakers"] = LAYOUTS[layout]
        return code, want, call

    def op_configure_hrtf(self, table, which, images):
        # rvb_capi.h, rvb_ir_configure_hrtf: "table == NULL: the table of this context's previous rvb_ir_configure_hrtf call stays on the
        # device ...; RVB_ERR_STATE if there is none"; rvb_attenuate_hrtf*: "a following rvb_ir_configure_hrtf with table == NULL
        # returns RVB_ERR_STATE"; "A call with a table that fails with RVB_ERR_STATE because nothing is traced has uploaded its table"
        if table is None and self.hrtf_table not in ("T", "U"):
            return STATE, None, {"mic": (0.0, 0.0, 0.0), "images": self.w.image_lists["none"], "table": None}
        if table is not None:
            self.hrtf_table = table
        code, want, call = self._configure("hrtf", self.hrtf_table, which, images)
        call["table"] = self.w.hrtf[table] if table is not None else None
        return code, want, call

    def op_time_range_begin(self):
        # rvb_capi.h, rvb_ir_time_range_begin: "Optional first half of rvb_ir_time_range"
        return (OK if self.cfg is not None else STATE), None, {}

    def op_time_range(self):
        if self.cfg is None:
            return STATE, None, {}
        return OK, self.w.time_range(self.chans()), {}

    def _geometry(self, sample_rate, predelay, nbins):
        """The call's (predelay, sample_rate, nbins); without a configuration the last one's (the call is refused)."""
        if self.cfg is not None:
            seconds, n, cls = self.w.geometry(self.chans(), sample_rate, predelay, nbins)
            self.geometry = (seconds, sample_rate, n)
            return cls
        return None

    def op_accumulate(self, mode, sample_rate, predelay, nbins, ontop):
        """ontop False: a zeroed histogram of the drawn geometry.  True: on top of the previous accumulate's histogram, with ITS predelay,
        rate and nbins (a histogram has one geometry: the drawn one is not used).  "same": a zeroed histogram of the previous geometry.
        Where the previous histogram has another channel count (or there is none) the call falls back to ontop False."""
        reuse = bool(ontop) and self.cfg is not None and self.hist_geometry is not None and self.hist_geometry[0] == self.nch
        if reuse:
            cls, self.geometry = "reused", self.hist_geometry[1:]
        else:
            cls = self._geometry(sample_rate, predelay, nbins)
        seconds, rate, n = self.geometry
        fresh = ontop is not True or not reuse or self.hist is None or self.hist.shape != (self.nch, 8, n)
        call = {"predelay": seconds, "sample_rate": rate, "nbins": n, "nch": self.nch, "fresh": fresh, "class": cls}
        if fresh:
            self.hist = np.zeros((self.nch, 8, n), np.float32)
        # rvb_capi.h, the fused stage: "1. rvb_ir_configure_*" comes first: STATE without a configuration
        if self.cfg is None:
            return STATE, None, call
        # "RVB_IR_EXACT continues, bin by bin, the reference's serial left-to-right float sum from the values d_histogram holds"
        call["fixed"] = self.w.accumulate(self.hist, self.chans(), seconds, rate)
        self.hist_geometry = (self.nch, seconds, rate, n)
        # rvb_ir_exact_prepare: "rvb_ir_accumulate in either mode and with any nbins ... voids it"
        self.prepared = None
        return OK, self.hist, call

    def op_prepare(self, sample_rate, predelay, nbins):
        cls = self._geometry(sample_rate, predelay, nbins)
        seconds, rate, n = self.geometry
        call = {"predelay": seconds, "sample_rate": rate, "nbins": n, "class": cls}
        if self.cfg is None:
            return STATE, None, call
        # rvb_capi.h, rvb_ir_exact_prepare: "everything that does not depend on what the histogram holds"; a second one replaces the list
        self.prepared = (self.cfg, self.rec, seconds, rate, n)
        self.prepared_nbins = n
        return OK, None, call

    def op_fold(self, part):
        """two uneven ranges: [0, nbins // 3) and [nbins // 3, nbins)"""
        n = self.prepared_nbins
        b0, b1 = (0, n // 3) if part == 0 else (n // 3, n)
        fresh = self.hist is None or self.hist.shape != (self.nch, 8, n)
        call = {"nbins": n, "b0": b0, "b1": b1, "nch": self.nch, "fresh": fresh}
        if fresh:
            self.hist = np.zeros((self.nch, 8, n), np.float32)
        # rvb_capi.h, rvb_ir_exact_fold: STATE once anything has voided the list, and "for an nbins other than the prepared one"
        if self.prepared is None:
            return STATE, None, call
        cfg, rec, seconds, rate, _ = self.prepared
        # "bins [bin_begin, bin_end): each bin's impulses added in impulse order on top of what d_histogram holds"
        self.w.accumulate(self.hist, self.w.channels(rec, cfg), seconds, rate, b0, b1)
        return OK, self.hist, call

    def op_decay_curve(self):
        # rvb_capi.h, the decay calls: "none of them voids an IR configuration or a prepared exact list or touches a record"
        return OK, None, {}

    def op_grad_map(self):
        """rvb_reshade_grad_map with all-zero weights over 64 bins at 8192 Hz: a state operation — every entry of the map must be written,
        and with zero weights every entry is exactly 0."""
        call = {"skip": self.scene is None}           # (no scene: no map to hand over, and the walks pass no null pointer)
        if self.scene is None:
            return OK, None, call
        # rvb_capi.h, rvb_reshade_grad_map: "RVB_ERR_STATE for nothing traced, a last trace made without RVB_KEEP_LISTENER, the scene or the
        # directions changed since, no IR configuration, the HRTF model, which != RVB_IR_DIFFUSE, more than 8 channels"; "A failed call
        # writes nothing and leaves everything as it was"
        if self.rec is None or not self.kept & capi.KEEP_LISTENER or self.cfg is None or self.cfg.kind == "hrtf" \
                or self.cfg.which != capi.IR_DIFFUSE or self.nch > 8:
            return STATE, None, call
        # "It uses the sort buffers, so like rvb_ir_accumulate it voids a prepared exact list"; "the IR configuration stays"; "Changes no
        # byte of the records, of the direct slot, of the candidates or of the time range"; "EVERY entry is written"
        self.prepared = None
        return OK, "zeros", call

    # ---- the materialised calls ------------------------------------------------------------------------------------------------------
    def op_flatten_query(self, array, sample_rate):
        # rvb_capi.h, rvb_flatten: "Called with out == NULL it reports *nbins"; rvb_ir_exact_prepare: "rvb_flatten* ... voids it"
        self.prepared = None
        return OK, self.w.flatten(array, sample_rate).shape[1], {"array": self.w.flat_array(array)}

    def op_flatten_fill(self, array, sample_rate):
        # rvb_flatten: whether the fill finds the query's keys or uploads again, "Bit-exact with the reference's serial summation order"
        self.prepared = None
        want = self.w.flatten(array, sample_rate)
        return OK, want, {"array": self.w.flat_array(array), "capacity": want.shape[1]}

    def op_attenuate_speaker(self, array, speaker):
        # rvb_capi.h: "rvb_attenuate_speaker* leave the IR configuration, a prepared exact list and the sort buffers alone"
        d, k = ae.EDGE_SPEAKERS[speaker]
        return OK, self.w.attenuate(array, speaker), {"records": self.w.att_arrays[array], "direction": d, "coefficient": k}

    def op_attenuate_hrtf(self, array, ear):
        # rvb_capi.h: "rvb_attenuate_hrtf* ... void the IR configuration (whichever model it names) and a prepared exact list, and a
        # following rvb_ir_configure_hrtf with table == NULL returns RVB_ERR_STATE"
        self.cfg, self.prepared, self.hrtf_table = None, None, "one"
        return OK, self.w.attenuate(array, ("ear", ear)), {"records": self.w.att_arrays[array], "table": self.w.hrtf["T"][ear]}


FETCHES = (("get_raw_diffuse",), ("get_direct",), ("get_image_candidates",))
CHECKPOINT = FETCHES + (("configure_speakers", "s2", capi.IR_ALL, "all"), ("time_range",), ("accumulate", capi.IR_EXACT, 44100.0, "min", "full", False))


class Disagreement(AssertionError):
    pass


class Walk:
    """A context-like object and the model, operation by operation.  `ctx` has the methods of capi.Context and, beside them,
    flatten_query / flatten_fill (the two halves of rvb_flatten), ir_time_range_begin, and a get_raw_diffuse that returns MAX_RECORDS
    records whatever the context believes to hold.  Histograms are torch tensors on `device`."""

    def __init__(self, world, ctx, device, label="", model=None, before=(), keep_histograms=False):
        """model: the one that has followed `ctx` since it was created, where the context is older than this walk; before: the operations
        it has seen until now (a failure prints them in front of the walk's own, so that the list replays on a new context)"""
        import torch
        self.torch, self.w, self.ctx, self.device, self.label = torch, world, ctx, device, label
        self.m = model if model is not None else ContextModel(world)
        self.m.hist = self.m.hist_geometry = None          # (histograms are the walk's own: the first call that needs one makes it)
        self.before, self.ops, self.backing, self.hist = tuple(before), [], None, None
        self.seen, self.events = collections.Counter(), []
        self.histograms = [] if keep_histograms else None  # (really on top, what the device held) of every accumulate

    def fail(self, what):
        raise Disagreement("%s step %d, %r: %s\nreplay(%r)" % (self.label, len(self.ops) - 1, self.ops[-1], what, list(self.before) + self.ops))

    def run(self, ops):
        for op in ops:
            self.step(tuple(op))
        return self

    def step(self, op, after_refusal=False):
        self.ops.append(op)
        code, want, call = self.m.apply(op)
        try:
            got, rc = getattr(self, "call_" + op[0])(op, call), capi.OK
        except capi.RvbError as e:
            got, rc = None, e.code
        if rc != code:
            self.fail("returned code %d, the model has %d" % (rc, code))
        self.seen[op[0] if code == capi.OK else (op[0], code)] += 1
        if code == capi.OK:
            self.note(op, call)
            self.compare(op, got, want, call)
        elif not after_refusal and self.m.rec is not None:
            for fetch in FETCHES:                 # "A failed call leaves the results as they were"
                self.step(fetch, True)

    def note(self, op, call):
        """What the coverage conditions of tests/test_context_model_host.py count: sizes of the grow-only buffers as the walk goes."""
        m = self.m
        if op[0] in ("trace", "trace_pairs"):
            self.events.append(("records", len(m.rec.mics) * m.rec.ndirs * m.rec.nrefl, m.rec.nrefl % 32 == 0))      # (count, 16-bit key runs)
        elif op[0] in ("configure_speakers", "configure_hrtf"):
            self.events.append(("images", len(call["images"]), m.cfg.kind))
        elif op[0] == "prepare" or (op[0] == "accumulate" and (op[1] == capi.IR_EXACT or m.nch > 8)):
            self.events.append(("keys", m.chans()[0].shape[0] * (2 if m.cfg.kind == "hrtf" else 1)))

    # ---- comparisons: bit for bit, padding included; RVB_IR_FAST within fast_bound ---------------------------------------------------
    def compare(self, op, got, want, call):
        name = op[0]
        if name == "get_raw_diffuse":
            n = want.shape[0]
            if not (same_records(got[:n], want) and not got[:n]["pad"].any() and not got[:n]["position"][:, 3].any()):
                self.fail("the diffuse records differ from the oracle's (%d records)" % n)
            if got[n:].view(np.uint32).any():
                self.fail("records written behind the %d of the trace" % n)
        elif name == "get_direct":
            if not same_records(got, want) or got["pad"].any():
                self.fail("the direct slot differs: got time %r, the oracle has %r" % (got["time"].tolist(), want["time"].tolist()))
        elif name == "get_image_candidates":
            same = got.shape == want.shape and all(np.array_equal(got[f], want[f]) for f in ("ray", "slot", "index")) \
                and same_records(got["impulse"], want["impulse"])
            if not same:
                self.fail("the candidates differ: %d, the oracle has %d" % (got.shape[0], want.shape[0]))
        elif name == "time_range":
            if (np.float32(got[0]), np.float32(got[1])) != (np.float32(want[0]), np.float32(want[1])):
                self.fail("time range %r, the oracle has %r" % (got, want))
        elif name in ("accumulate", "fold"):
            got = self.read_hist()
            if name == "accumulate":
                if not call["fresh"] and call["nbins"] > 1:
                    self.seen["on top"] += 1
                if self.histograms is not None:
                    self.histograms.append((not call["fresh"], got.copy()))
            if name == "accumulate" and op[1] == capi.IR_FAST:
                self.seen["fast", call["class"]] += 1
                excess = np.abs(got.astype(np.float64) - want) - fast_bound(want, call["fixed"], call["sample_rate"])
                if not (excess <= 0).all():
                    self.fail("RVB_IR_FAST: %d band-bins outside fast_bound" % np.count_nonzero(excess > 0))
                self.m.hist = got.copy()            # what the device holds is what a later call continues from
            else:
                if name == "accumulate":
                    self.seen["exact", call["class"]] += 1
                if not np.array_equal(got.view(np.uint32), want.view(np.uint32)):
                    ch, band, bin_ = np.argwhere(got.view(np.uint32) != want.view(np.uint32))[0]
                    self.fail("histogram %s: channel %d band %d bin %d: got %r, the oracle chain has %r (%d band-bins differ)"
                              % (got.shape, ch, band, bin_, got[ch, band, bin_], want[ch, band, bin_], np.count_nonzero(got != want)))
        elif name == "decay_curve":
            if self.hist is not None and not np.array_equal(self.read_hist()[:self.m.hist.shape[0]].view(np.uint32), self.m.hist.view(np.uint32)):
                self.fail("rvb_decay_curve changed its histogram")
        elif name == "grad_map":
            if want is not None and got.view(np.uint32).any():
                self.fail("rvb_reshade_grad_map with zero weights: %d entries of the map are not 0 (or were not written)" % np.count_nonzero(got.view(np.uint32)))
        elif name == "flatten_query":
            if got != want:
                self.fail("rvb_flatten reports %d bins, the oracle has %d" % (got, want))
        elif name == "flatten_fill":
            if got.shape != want.shape or not np.array_equal(got.view(np.uint32), want.view(np.uint32)):
                self.fail("rvb_flatten: %d of %s band-bins differ from the oracle's" % (np.count_nonzero(got != want) if got.shape == want.shape else -1, want.shape))
        elif name in ("attenuate_speaker", "attenuate_hrtf"):
            if not (np.array_equal(got["volume"].view(np.uint32), want["volume"].view(np.uint32)) and np.array_equal(got["time"].view(np.uint32), want["time"].view(np.uint32))
                    and not got["pad"].any()):
                self.fail("the attenuated records differ from the oracle's")

    # ---- histograms: room for MAX_CHANNELS channels whatever the context holds, so that no call can write past the buffer ----------
    def histogram(self, nch, nbins, fresh):
        if fresh or self.hist is None:
            self.backing = self.torch.zeros(MAX_CHANNELS * 8 * nbins, dtype=self.torch.float32, device=self.device)
            rows = max(nch, 1)                  # (never configured: the call is refused, and still gets a buffer that is none of null)
            self.hist = self.backing[:rows * 8 * nbins].view(rows, 8, nbins)
        return self.hist

    def read_hist(self):
        self.ctx.synchronize()
        return self.hist.cpu().numpy()

    # ---- the calls -------------------------------------------------------------------------------------------------------------------
    def call_set_scene(self, op, call):
        self.ctx.set_scene(call["scene"])

    def call_set_directions(self, op, call):
        self.ctx.set_directions(call["dirs"])

    def call_keep_paths(self, op, call):
        self.ctx.keep_paths(op[1] != 0, listener=bool(op[1] & capi.KEEP_LISTENER))

    def call_set_source_pattern(self, op, call):
        self.ctx.set_source_pattern(*((FACING, SHAPES) if op[1] else (None,)))

    def call_trace(self, op, call):
        self.ctx.trace(call["mics"][0], call["sources"][0], op[3], call["air"], op[5])

    def call_trace_pairs(self, op, call):
        self.ctx.trace_pairs(np.array(call["mics"], np.float32), np.array(call["sources"], np.float32), op[1], call["air"], op[3])

    def call_select_pair(self, op, call):
        self.ctx.select_pair(op[1])

    def call_reshade(self, op, call):
        self.ctx.reshade(call["surfaces"], call["air"])

    def call_relisten(self, op, call):
        self.ctx.relisten(np.array(call["mics"], np.float32))

    def call_get_raw_diffuse(self, op, call):
        return self.ctx.get_raw_diffuse()

    def call_get_direct(self, op, call):
        return self.ctx.get_direct()

    def call_get_image_candidates(self, op, call):
        return self.ctx.get_image_candidates()

    def call_configure_speakers(self, op, call):
        self.ctx.ir_configure_speakers(call["mic"], [d for d, _ in call["speakers"]], [k for _, k in call["speakers"]], op[2], call["images"])

    def call_configure_hrtf(self, op, call):
        self.ctx.ir_configure_hrtf(call["mic"], call["table"], self.w.facing, self.w.up, op[2], call["images"])

    def call_time_range_begin(self, op, call):
        self.ctx.ir_time_range_begin()

    def call_time_range(self, op, call):
        return self.ctx.ir_time_range()

    def call_accumulate(self, op, call):
        hist = self.histogram(call["nch"], call["nbins"], call["fresh"])
        self.ctx.ir_accumulate_tensor(call["predelay"], call["sample_rate"], call["nbins"], op[1], hist)

    def call_prepare(self, op, call):
        self.ctx.ir_exact_prepare(call["predelay"], call["sample_rate"], call["nbins"])

    def call_fold(self, op, call):
        hist = self.histogram(call["nch"], call["nbins"], call["fresh"])
        self.ctx.ir_exact_fold_tensor(call["nbins"], call["b0"], call["b1"], hist)

    def call_decay_curve(self, op, call):
        if self.hist is not None and self.hist.numel():
            self.ctx.decay_curve_tensor(self.hist)

    def call_grad_map(self, op, call):
        if call["skip"]:
            return None
        t, triangles = self.torch, self.w.scene(self.m.scene)[0].shape[0]
        weights = t.zeros(MAX_CHANNELS * 8 * 64, dtype=t.float32, device=self.device)
        out = t.full((triangles, 16), float("nan"), dtype=t.float32, device=self.device)
        self.ctx.reshade_grad_map(0.0, 8192.0, 64, weights.data_ptr(), out)
        return out.cpu().numpy()

    def call_flatten_query(self, op, call):
        return self.ctx.flatten_query(call["array"], op[2])

    def call_flatten_fill(self, op, call):
        return self.ctx.flatten_fill(call["array"], op[2], call["capacity"])

    def call_attenuate_speaker(self, op, call):
        return self.ctx.attenuate_speaker(ae.OBLIQUE["mic"], call["records"], call["direction"], call["coefficient"])

    def call_attenuate_hrtf(self, op, call):
        return self.ctx.attenuate_hrtf(ae.OBLIQUE["mic"], call["records"], call["table"], self.w.facing, self.w.up, op[2])


def replay(world, ctx, device, ops, label="replay", **more):
    """Runs a list of operations as a failing walk prints it."""
    return Walk(world, ctx, device, label, **more).run(ops)


def on_top_is_the_all_chain(walk):
    """DIRECTED["diffuse_then_images_on_top_is_the_all_chain"], run with keep_histograms: its last accumulate went on top of the diffuse
    one, and what the device then held is, bit for bit, what it held after the ALL configuration's accumulate on a zeroed histogram."""
    (top0, all_), (top1, _), (top2, both) = walk.histograms
    return (top0, top1, top2) == (False, False, True) and all_.shape == both.shape and all_.shape[2] > 1 and all_.any() \
        and np.array_equal(all_.view(np.uint32), both.view(np.uint32))


# ---- directed sequences ------------------------------------------------------------------------------------------------------------
D, I, A = capi.IR_DIFFUSE, capi.IR_IMAGES, capi.IR_ALL
EXACT, FAST = capi.IR_EXACT, capi.IR_FAST
START = (("set_scene", "cathedral"), ("set_directions", 130), ("trace", 0, 0, 24, "A", 0))
S2 = ("configure_speakers", "s2", A, "all")


def _classes(configure, mode):
    ops = list(START) + [configure]
    for k, cls in enumerate(NBINS):
        ops.append(("accumulate", mode, RATES[k % 2], PREDELAYS[k % 3], cls, False))
    return tuple(ops)


DIRECTED = {
    # (first: on the GPU the module's context is new here, so the refusals of a context without a scene are the device's)
    "calls_before_a_scene_are_refused": (
        ("set_directions", 5), ("trace", 0, 0, 1, "A", 0), ("trace_pairs", 1, "A", 0)) + FETCHES + (
        ("select_pair", 0), S2, ("configure_hrtf", "T", A, "none"), ("time_range_begin",), ("time_range",),
        ("accumulate", EXACT, 44100.0, "zero", "full", False), ("prepare", 44100.0, "zero", "full"), ("fold", 0), ("reshade", "own", "A"),
        ("relisten", 0), ("decay_curve",), ("set_scene", "shoebox"), ("trace", 0, 0, 1, "A", 0)) + CHECKPOINT,
    "prepare_then_decay_curve_flatten_attenuate": START + (
        S2, ("prepare", 44100.0, "min", "full"), ("decay_curve",), ("fold", 0), ("fold", 1),
        ("prepare", 44100.0, "min", "full-1"), ("flatten_query", "tiny", 44100.0), ("fold", 0),
        ("prepare", 8192.0, "zero", "full"), ("attenuate_speaker", "edge", 4), ("fold", 1), ("fold", 0),
        ("prepare", 44100.0, "above", "p"), ("accumulate", EXACT, 44100.0, "above", "p", False), ("fold", 0),
        ("prepare", 44100.0, "above", "p"), ("accumulate", FAST, 44100.0, "above", "p+1", False), ("fold", 0),
        ("prepare", 44100.0, "min", "full"), S2, ("fold", 0),
        ("prepare", 44100.0, "min", "full"), ("select_pair", 0), ("fold", 0)),
    "flatten_query_then_other_calls_then_fill": START + (
        ("flatten_query", "edge", 8192.0), ("trace", 1, 0, 32, "A", 0), ("flatten_fill", "edge", 8192.0),
        ("flatten_query", "edge", 44100.0), S2, ("flatten_fill", "edge", 44100.0),
        ("flatten_query", "big", 44100.0), ("accumulate", EXACT, 44100.0, "min", "full", False), ("flatten_fill", "big", 44100.0),
        ("flatten_query", "tiny", 44100.0), ("accumulate", EXACT, 8192.0, "zero", "full", False), ("flatten_fill", "tiny", 44100.0),
        ("flatten_query", "big", 8192.0), ("flatten_query", "tiny", 8192.0), ("flatten_fill", "tiny", 8192.0), ("flatten_fill", "tiny", 8192.0),
        ("flatten_fill", "big", 8192.0), ("flatten_query", "edge", 8192.0), ("accumulate", FAST, 8192.0, "min", "full", False),
        ("flatten_fill", "edge", 8192.0)),
    "hrtf_table_after_a_one_ear_attenuate": START + (
        ("attenuate_hrtf", "bnd", 0), ("configure_hrtf", None, A, "all"), ("configure_hrtf", "T", A, "all"), ("time_range",), ("prepare", 44100.0, "min", "full"),
        ("attenuate_hrtf", "bnd", 1), ("fold", 0), ("time_range",), ("accumulate", EXACT, 44100.0, "min", "full", False),
        ("configure_hrtf", None, A, "all"), ("configure_hrtf", "U", D, "none"), ("accumulate", EXACT, 44100.0, "min", "full", False),
        ("configure_hrtf", None, A, "first3"), ("time_range",), ("accumulate", EXACT, 8192.0, "zero", "full", False),
        S2, ("attenuate_hrtf", "bnd", 0), ("time_range",), ("accumulate", EXACT, 44100.0, "min", "full", False)),
    "hrtf_range_enqueued_then_another_configuration": START + (
        ("configure_hrtf", "T", A, "all"), ("time_range_begin",), ("configure_hrtf", None, I, "first3"), ("time_range",),
        ("time_range_begin",), ("time_range",), ("time_range_begin",), ("configure_hrtf", "U", D, "none"), ("time_range",)),
    "speakers_9_2_9_with_another_layout": START + (
        ("configure_speakers", "s9", A, "all"), ("accumulate", EXACT, 44100.0, "min", "full", False),
        S2, ("accumulate", EXACT, 44100.0, "min", "full", False),
        ("configure_speakers", "s9r", A, "all"), ("accumulate", EXACT, 44100.0, "min", "full", False),
        ("configure_hrtf", "T", A, "all"), ("accumulate", EXACT, 44100.0, "min", "full", False),
        ("configure_speakers", "s9", D, "none"), ("accumulate", FAST, 44100.0, "zero", "full", False)),
    "images_40_then_3_then_40_others": START + (
        ("configure_speakers", "s2", I, "e40a"), ("time_range",), ("accumulate", EXACT, 44100.0, "min", "full", False),
        ("configure_speakers", "s2", I, "first3"), ("time_range",), ("accumulate", EXACT, 44100.0, "min", "full", False),
        ("configure_speakers", "s2", I, "e40b"), ("time_range",), ("accumulate", EXACT, 44100.0, "min", "full", False),
        ("configure_hrtf", "T", A, "e40a"), ("time_range",), ("accumulate", EXACT, 44100.0, "min", "full", False),
        ("configure_speakers", "s9", I, "none"), ("time_range",), ("accumulate", EXACT, 44100.0, "zero", "full", False)),
    "select_pair_then_reshade": (
        ("set_scene", "cathedral"), ("set_directions", 130), ("keep_paths", 1), ("trace_pairs", 24, "A", 1000)) + FETCHES + (
        ("select_pair", 3), ("select_pair", 2), ("get_direct",), S2, ("time_range",), ("prepare", 44100.0, "min", "full"),
        ("select_pair", 1), ("fold", 0), ("time_range",), ("select_pair", 2), S2, ("reshade", "B", "B"), ("time_range",),
        ("accumulate", EXACT, 44100.0, "min", "full", False), ("get_direct",), S2, ("time_range",),
        ("accumulate", EXACT, 44100.0, "min", "full", False)) + FETCHES,
    "reshade_that_mutes_a_surface_moves_the_range": (
        ("set_scene", "cathedral"), ("set_directions", 509), ("keep_paths", 1), ("trace", 0, 0, 24, "A", 0),
        ("configure_speakers", "s2", D, "none"), ("time_range",), ("reshade", "short", "B"), ("time_range",), ("reshade", "B", "B"),
        ("time_range",), ("configure_speakers", "s2", D, "none"), ("time_range",), ("set_source_pattern", 1), ("reshade", "own", "A"),
        ("configure_speakers", "s2", D, "none"), ("time_range",)) + FETCHES + (("set_source_pattern", 0), ("reshade", "own", "A")) + FETCHES,
    "diffuse_then_images_on_top_is_the_all_chain": START + (
        S2, ("accumulate", EXACT, 44100.0, "min", "full", False),                                        # the ALL chain, which sets the geometry
        ("configure_speakers", "s2", D, "none"), ("accumulate", EXACT, 44100.0, "min", "full", "same"),   # zeroed, that geometry
        ("configure_speakers", "s2", I, "all"), ("accumulate", EXACT, 44100.0, "min", "full", True)),     # on top: on_top_is_the_all_chain()
    "shrink_and_grow_with_keeping_on": (
        ("set_scene", "cathedral"), ("keep_paths", 3), ("set_directions", 509), ("trace", 0, 0, 70, "A", 0)) + CHECKPOINT + (
        ("relisten", 0),) + CHECKPOINT + (
        ("set_scene", "shoebox"), ("set_directions", 5), ("trace", 0, 0, 1, "A", 0)) + CHECKPOINT + (("relisten", 0),) + CHECKPOINT + (
        ("set_scene", "cathedral"), ("set_directions", 130), ("trace", 1, 1, 64, "B", 0)) + CHECKPOINT + (("relisten", 0),) + CHECKPOINT,
    "keeping_switched_on_after_the_trace": (("keep_paths", 0),) + START + (
        ("reshade", "B", "B"), ("keep_paths", 1), ("reshade", "B", "B"), ("relisten", 0), ("trace", 0, 0, 24, "A", 0), ("reshade", "B", "B"),
        ("relisten", 0)) + FETCHES + (("keep_paths", 3), ("trace", 0, 0, 24, "A", 0), ("relisten", 1), ("relisten", 0), ("reshade", "B", "A")) + FETCHES + (
        ("keep_paths", 0), ("reshade", "own", "A"), ("relisten", 0)) + FETCHES + (
        ("keep_paths", 3), ("trace", 0, 0, 24, "A", 0), ("keep_paths", 0), ("keep_paths", 3), ("reshade", "B", "B"), ("trace", 1, 0, 32, "A", 0),
        ("keep_paths", 0), ("trace", 1, 0, 32, "A", 0), ("keep_paths", 3), ("relisten", 0)) + FETCHES,
    "a_changed_scene_or_ray_set_voids_everything": START + FETCHES + (
        S2, ("prepare", 44100.0, "min", "full"), ("set_directions", 509), ("fold", 0), ("time_range",), ("accumulate", EXACT, 44100.0, "min", "full", False),
        ("select_pair", 0), S2) + FETCHES + (("trace", 0, 0, 1, "A", 0),) + CHECKPOINT + (
        ("set_scene", "shoebox"), ("time_range",), ("prepare", 44100.0, "min", "full")) + FETCHES + (("trace", 0, 0, 32, "A", 0),) + CHECKPOINT,
    "a_second_trace_is_fetched_afresh": START + FETCHES + (
        S2, ("time_range",), ("trace", 1, 1, 24, "B", 1000), ("time_range",)) + CHECKPOINT + (
        ("trace_pairs", 24, "A", 0), ("select_pair", 2)) + FETCHES + (("trace", 0, 0, 24, "A", 0),) + CHECKPOINT + (
        ("trace_pairs", 1, "A", 0), ("select_pair", 2), ("trace_pairs", 1, "B", 0)) + FETCHES + (("keep_paths", 3), ("trace", 0, 0, 24, "A", 0)) + FETCHES + (
        ("relisten", 0),) + FETCHES + (("reshade", "B", "B"),) + FETCHES,
    "the_gradient_map_uses_the_sort_buffers": (
        ("set_scene", "cathedral"), ("keep_paths", 3), ("set_directions", 130), ("trace", 0, 0, 24, "A", 0), ("grad_map",),
        ("configure_speakers", "s2", D, "none"), ("prepare", 44100.0, "min", "full"), ("grad_map",), ("fold", 0), ("time_range",),
        ("flatten_query", "big", 8192.0), ("grad_map",), ("flatten_fill", "big", 8192.0)) + FETCHES + (
        ("configure_hrtf", "T", D, "none"), ("grad_map",), ("configure_speakers", "s9", D, "none"), ("grad_map",), S2, ("grad_map",),
        ("keep_paths", 1), ("trace", 0, 0, 24, "A", 0), ("configure_speakers", "s2", D, "none"), ("grad_map",),
        ("keep_paths", 3), ("trace", 0, 0, 24, "A", 0), ("configure_speakers", "s2", D, "none"), ("set_directions", 130), ("grad_map",)),
    "nbins_classes_speakers2_exact": _classes(S2, EXACT),
    "nbins_classes_speakers9_exact": _classes(("configure_speakers", "s9", A, "all"), EXACT),
    "nbins_classes_hrtf_exact": _classes(("configure_hrtf", "T", A, "all"), EXACT),
    "nbins_classes_speakers2_fast": _classes(S2, FAST),
    "nbins_classes_hrtf_fast": _classes(("configure_hrtf", "T", A, "all"), FAST),
}

# ---- seeded walks --------------------------------------------------------------------------------------------------------------------
SEEDS = tuple(range(1, 13))
WALK_LENGTH = 60


def seeded_walk(seed, length=WALK_LENGTH):
    """`length` drawn operations (checkpoints, which are several, count as one).  Every walk begins on the large scene at the largest
    size and alternates between large and small traces, and between the two key modes of the trace, so that every buffer shrinks and
    grows again; in between the operations are drawn from all menus, refused ones included.  Nine question blocks — a small kept trace and
    one sequence each about a changed scene, changed rays, a prepared list, keeping, the HRTF table, the pairs, a flatten query with an
    accumulate on top, a new configuration, the gradient map — stand at drawn places, and behind any drawn operation a full checkpoint
    follows with probability 0.15."""
    rng = np.random.default_rng(seed)
    pick = lambda menu: menu[int(rng.integers(len(menu)))]
    ops = [("set_directions", 5), ("trace", 0, 0, 1, "A", 0), ("get_direct",), ("select_pair", 0),         # no scene yet: refused
           ("set_scene", "cathedral"), ("keep_paths", int(pick((0, 1, 3)))), ("set_directions", 509), ("trace", 0, 0, int(pick((70, 24))), "A", 0)]
    # the sizes of the traces to come: large, small, large ...; 16-bit key runs (32, 64) and 32-bit keys (1, 24, 70) in turn
    sizes = [(5, 32), (509, 64), (5, 1), (130, 70), (130, 32), (509, 24)]
    rng.shuffle(sizes)
    sizes = [(5, 32), (509, 70)] + sizes
    layouts = ["s9", "T", "s2", "U", "s9r"]                     # speakers -> hrtf -> speakers at the least
    geometry = lambda: (float(pick(RATES)), pick(PREDELAYS), pick(NBINS))
    probes = dict(zip((int(x) for x in rng.choice(np.arange(6, length), 9, replace=False)), range(9)))
    drawn = 0
    while drawn < length:
        drawn += 1
        if drawn in probes:
            # every walk asks each of these questions once, somewhere, behind a small kept trace of its own
            g, array, rate = geometry(), pick(FLAT_ARRAYS), float(pick(RATES))
            ops.extend((("keep_paths", 3), ("set_directions", int(pick((5, 130)))), ("trace", int(pick((0, 1))), 0, int(pick((1, 24, 32))), pick(AIRS), 0)))
            ops.extend((
                (("get_direct",), S2, ("set_scene", pick(SCENES))) + FETCHES + (("accumulate", EXACT) + g + (False,),),
                (("get_direct",), S2, ("set_directions", int(pick(NDIRS)))) + FETCHES + (("time_range",), ("accumulate", EXACT) + g + (False,)),
                (S2, ("prepare",) + g, ("flatten_query", array, rate), ("fold", 0), ("prepare",) + g, ("select_pair", 0), ("fold", 0),
                 S2, ("prepare",) + g, ("accumulate", EXACT) + g + (False,), ("fold", 1)),
                (("keep_paths", 0), ("reshade", "B", "B"), ("relisten", 0)),
                (("configure_hrtf", "T", A, "all"), ("time_range_begin",), ("configure_hrtf", None, I, "first3"), ("time_range",),
                 ("configure_hrtf", "T", A, "all"), ("prepare",) + g, ("attenuate_hrtf", "bnd", int(pick((0, 1)))), ("fold", 0),
                 ("accumulate", EXACT) + g + (False,), ("configure_hrtf", None, A, "first3")),
                (("trace_pairs", int(pick((1, 24))), pick(AIRS), int(pick(OFFSETS))), ("select_pair", 2), ("get_direct",),
                 ("trace_pairs", int(pick((1, 24))), pick(AIRS), 0), ("get_direct",), S2, ("time_range",)),
                (S2, ("flatten_query", array, rate), ("accumulate", EXACT, rate, "min", "full", False), ("flatten_fill", array, rate),
                 ("configure_speakers", "s2", I, "all"), ("accumulate", EXACT, rate, "min", "full", True)),
                (S2, ("prepare",) + g, ("configure_speakers", pick(("s2", "s9")), int(pick(WHICH)), pick(IMAGES)), ("fold", int(pick((0, 1))))),
                (("configure_speakers", "s2", D, "none"), ("flatten_query", "big", rate), ("grad_map",), ("flatten_fill", "big", rate),
                 ("prepare",) + g, ("grad_map",), ("fold", 0)),
            )[probes[drawn]])
            continue
        r = rng.random()
        if (r < 0.09 or drawn in (8, 24, 40)) and sizes:               # (three of them at fixed places: no seed goes without)
            n, nrefl = sizes.pop(0)
            if rng.random() < 0.35:
                ops.append(("set_scene", pick(SCENES)))
            ops.append(("keep_paths", int(pick((0, 1, 3, 3)))))
            ops.append(("set_directions", n))
            if rng.random() < 0.3:
                ops.append(("trace_pairs", nrefl, pick(AIRS), int(pick(OFFSETS))))
            else:
                ops.append(("trace", int(pick((0, 1))), int(pick((0, 1))), nrefl, pick(AIRS), int(pick(OFFSETS))))
            ops.extend(CHECKPOINT)
            if rng.random() < 0.5 or drawn in (8, 24, 40):          # speakers (the checkpoint's) -> hrtf -> speakers (the next one's)
                ops.extend((("configure_hrtf", pick(("T", "U")), int(pick(WHICH)), pick(IMAGES)), ("time_range",), ("accumulate", EXACT) + geometry() + (False,)))
        elif r < 0.13:
            ops.append(("trace", int(pick((0, 1))), int(pick((0, 1))), int(pick(NREFL)), pick(AIRS), int(pick(OFFSETS))))
        elif r < 0.16:
            ops.append(("trace_pairs", int(pick(NREFL)), pick(AIRS), int(pick(OFFSETS))))
        elif r < 0.20:
            ops.append(("select_pair", int(pick((0, 1, 2, 2)))))
        elif r < 0.27:
            ops.append(("reshade", pick(("own", "B", "B", "short")), pick(AIRS)))
            if rng.random() < 0.5:
                ops.extend(CHECKPOINT)
        elif r < 0.33:
            ops.append(("relisten", int(rng.random() < 0.15)))
            if rng.random() < 0.5:
                ops.extend(CHECKPOINT)
        elif r < 0.36:
            ops.append(("keep_paths", int(pick((0, 1, 3)))))
        elif r < 0.39:
            ops.append(("set_source_pattern", int(pick((0, 1)))))
        elif r < 0.41:
            ops.append(pick((("set_directions", int(pick(NDIRS))), ("set_scene", pick(SCENES)))))
        elif r < 0.53:
            layout = layouts.pop(0) if layouts and rng.random() < 0.6 else pick(("s2", "s9", "s9r", "T", "U", None))
            which, images = int(pick(WHICH)), pick(IMAGES)
            ops.append(("configure_hrtf", layout, which, images) if layout in HRTF_TABLES else ("configure_speakers", layout, which, images))
        elif r < 0.58:
            ops.extend(pick(((("time_range",),), (("time_range_begin",), ("time_range",)), (("time_range_begin",),))))
        elif r < 0.70:
            mode = int(pick((EXACT, EXACT, FAST)))
            ops.append(("accumulate", mode) + geometry() + (bool(mode == EXACT and rng.random() < 0.4),))
        elif r < 0.78:
            # a prepared list, one call that leaves it alone or voids it, a fold
            g, array, rate = geometry(), pick(FLAT_ARRAYS), float(pick(RATES))
            ops.append(("prepare",) + g)
            ops.extend(pick(((), (("fold", 0),), (("decay_curve",),), (("flatten_query", array, rate),), (("flatten_fill", array, rate),),
                             (("attenuate_speaker", "edge", 2),), (("attenuate_hrtf", "bnd", 1),), (("select_pair", 0),), (S2,),
                             (("accumulate", EXACT) + g + (False,),), (("accumulate", FAST) + g + (False,),), (("time_range",),))))
            ops.append(("fold", int(pick((0, 1)))))
        elif r < 0.79:
            ops.append(("fold", int(pick((0, 1)))))
        elif r < 0.85:
            array, rate = pick(FLAT_ARRAYS), float(pick(RATES))
            ops.extend(pick(((("flatten_query", array, rate),), (("flatten_fill", array, rate),),
                             (("flatten_query", array, rate), ("flatten_fill", array, rate), ("flatten_fill", array, rate)))))
        elif r < 0.88:
            ops.append(("flatten_fill", pick(FLAT_ARRAYS), float(pick(RATES))))
        elif r < 0.91:
            ops.append(("attenuate_speaker", pick(ATT_ARRAYS), int(rng.integers(len(ae.EDGE_SPEAKERS)))))
        elif r < 0.94:
            ops.append(("attenuate_hrtf", "bnd", int(pick((0, 1)))))              # (the speaker edges hold positions the HRTF rows are not defined for)
        elif r < 0.96:
            ops.append(pick((("decay_curve",), ("grad_map",))))
        else:
            ops.extend(FETCHES)
        if rng.random() < 0.15:                                       # a full checkpoint behind any operation, by the walk's own choice
            ops.extend(CHECKPOINT)
    return tuple(ops)
