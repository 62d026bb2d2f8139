"""The walks of tests/context_model.py can see what they are for — shown without a GPU.

LedgerContext has the method surface of capi.Context over the CPU oracle (in the manner of tests/oracle_tracer.py) and keeps the same
caches and flags as rvb_ctx, function by function as csrc/ does: the fetched small block, the tenant of the sort buffers (the keys of a
flatten size query or a prepared list: IrState of csrc/ir_state.h) beside what the buffers really hold, the trace's flags and selected
pair (TraceState of csrc/trace_state.h; its live count has no reader among the walks and is not modelled), its own copy of the images, the
ear count of the table, the kept state, the selected pair.
`forget=<site>` leaves out exactly one invalidation of the code.  The conditions below: the model and the complete stand-in agree on
every walk; every forgotten invalidation is flagged by a directed sequence and by a quarter of the seeds; the seeds cover every
operation, every refusal and every nbins class, and every seed shrinks and grows every buffer."""
import collections

import numpy as np
import pytest

import context_model as cm
from context_model import Disagreement, Rec, Walk
from parallel_reverb_raytracer_amd import capi
from parallel_reverb_raytracer_amd.dtypes import IMPULSE

# the invalidation sites of csrc/, "function:what it clears" or "function:the transition of IrState / TraceState (or the composition of rvb_ctx) it calls"
FORGETS = (
    "ensure_sort_buffers:tenant", "configure_common:exact.valid", "configure_common:range_pending",
    "set_one_ear_table:hrtf_table_ears", "set_one_ear_table:drop_configuration", "drop_configuration:configured", "drop_configuration:exact.valid",
    "trace_finish:not fetched", "trace_finish:pair 0", "trace_finish:kept", "reshade:void_fetched_results",
    "relisten:void_fetched_results", "set_scene:traced", "set_directions:traced", "void_trace:drop_configuration", "keep_paths(0):release",
    "select_pair:drop_configuration", "accumulate:exact.valid", "flatten_fill:keys consumed",
)
# NOT SHOWN here: "share_scene: traced".  rvb_share_scene needs a second context and is no operation of the walks, so the stand-in has no
# such site and nothing here says that a walk would notice that line missing.


class LedgerContext:
    def __init__(self, world, forget=None):
        assert forget is None or forget in FORGETS, forget
        self.w, self.forget = world, forget
        self.scene = self.nrays = None
        self.traced, self.dev, self.npairs, self.ir_pair = False, None, 1, 0
        self.pattern = False
        self.keep, self.keep_listener, self.kept_valid, self.listener_valid, self.kept_rec = False, False, False, False, None
        self.small_valid, self.small_host = False, None
        self.ir_configured, self.model, self.which, self.images_host, self.images_key = False, None, capi.IR_ALL, np.zeros(0, IMPULSE), None
        self.nchannels = 0
        self.hrtf_table, self.hrtf_table_ears = None, 0
        self.range_pending, self.range_host = False, (0.0, 0.0)
        self.tenant, self.query, self.exact = "nothing", None, None   # IrState: "nothing" / "flatten query" / "exact list", and the two payloads
        self.sort_cap, self.sort_keys = 0, "nothing"                  # capacity of keys_a, and whose keys it really holds
        self._chans = {}

    def forgot(self, site):
        return self.forget == site

    @staticmethod
    def fail(code, text):
        raise capi.RvbError(code, text)

    def synchronize(self):
        pass

    # ---- ir_state.h ------------------------------------------------------------------------------------------------------------------
    def void_exact_list(self):
        if self.tenant == "exact list":
            self.tenant = "nothing"

    def drop_configuration(self):
        if not self.forgot("drop_configuration:configured"):
            self.ir_configured = False
        if not self.forgot("drop_configuration:exact.valid"):
            self.void_exact_list()

    # ---- context.hip -----------------------------------------------------------------------------------------------------------------
    def void_trace(self, site):
        if not self.forgot(site):
            self.traced = False
        if not self.forgot("void_trace:drop_configuration"):
            self.drop_configuration()

    def set_scene(self, scene):
        self.scene = next(name for name in cm.SCENES if self.w.scene(name) is scene)
        self.void_trace("set_scene:traced")

    def set_directions(self, directions):
        self.nrays = int(directions.shape[0])
        self.void_trace("set_directions:traced")

    def set_source_pattern(self, direction, shape=None):
        self.pattern = direction is not None

    # ---- trace.hip -------------------------------------------------------------------------------------------------------------------
    def void_fetched_results(self, site):
        """rvb_ctx::void_fetched_results: TraceState::records_rewritten — not fetched, pair 0 — and the configuration dropped"""
        if self.forgot(site):
            return
        self.small_valid = False
        self.ir_pair = 0
        self.drop_configuration()

    def _index(self, what, xyz):
        return next(i for i, v in enumerate(self.w.scenes[self.scene][what]) if np.allclose(v, xyz))

    def _air(self, air):
        return next(name for name in cm.AIRS if np.array_equal(self.w.air(name), np.asarray(air, np.float32)))

    def trace(self, mic, source, nreflections, air, ray_offset=0):
        self.trace_pairs([mic], [source], nreflections, air, ray_offset)

    def trace_pairs(self, mics, sources, nreflections, air, ray_offset=0):
        if self.scene is None:
            self.fail(capi.ERR_STATE, "rvb_trace: rvb_set_scene has not been called")
        if self.nrays is None:
            self.fail(capi.ERR_STATE, "rvb_trace: no directions")
        self.void_trace("trace_prepare:traced")                           # (no forget site: trace_finish sets it again)
        if not self.forgot("trace_finish:kept"):
            self.kept_valid = self.listener_valid = False                 # KeptState::trace_begins
        self.dev = Rec(self.scene, "own", self._air(air), tuple(self._index("mics", m) for m in mics),
                       tuple(self._index("sources", s) for s in sources), self.nrays, int(nreflections), int(ray_offset), self.pattern)
        if not self.forgot("trace_finish:kept"):                          # kept.take(): KeptState::trace_taken
            self.kept_valid, self.listener_valid = self.keep, self.keep and self.keep_listener
            if self.kept_valid:
                self.kept_rec = self.dev
        self.traced = True                                                # TraceState::finished: traced, its sizes, not fetched, pair 0
        self.npairs = len(self.dev.mics)
        if not self.forgot("trace_finish:not fetched"):                   # (... and the configuration dropped, as void_trace has already)
            self.small_valid = False
            self.drop_configuration()
        if not self.forgot("trace_finish:pair 0"):
            self.ir_pair = 0

    def select_pair(self, pair):
        if not self.traced:
            self.fail(capi.ERR_STATE, "rvb_ir_select_pair: nothing traced")
        if pair >= self.npairs:
            self.fail(capi.ERR_INVALID, "rvb_ir_select_pair: pair out of range")
        self.ir_pair = pair
        if not self.forgot("select_pair:drop_configuration"):
            self.drop_configuration()

    def _pair_diffuse(self):
        """ir_diffuse(): the slice of the selected pair — beyond the launch there is no record of this trace"""
        if self.ir_pair < len(self.dev.mics):
            return self.w.pair(self.dev, self.ir_pair)["diffuse"]
        return np.zeros(self.dev.ndirs * self.dev.nrefl, IMPULSE)

    def fetch_small(self):
        if self.small_valid:
            return
        ranges = []
        for p in range(self.npairs):
            d = self.w.pair(self.dev, p)["diffuse"]
            t = d["time"][(d["volume"] != 0).any(axis=1)]
            ranges.append((t[t != 0].min() if (t != 0).any() else None, t.max() if t.size else np.float32(0)))
        self.small_host = {"direct": [self.w.pair(self.dev, p)["direct"] for p in range(self.npairs)], "cand": self.w.candidates(self.dev), "range": ranges}
        self.small_valid = True

    def _of_pair(self, what):
        block = self.small_host[what]
        if self.npairs > 1:
            return block[self.ir_pair] if self.ir_pair < len(block) else block[0] if what == "range" else np.zeros(1, IMPULSE)
        return block[0]

    def get_raw_diffuse(self):
        if not self.traced:
            self.fail(capi.ERR_STATE, "rvb_get_diffuse: nothing traced")
        out = np.zeros(cm.MAX_RECORDS, IMPULSE)
        d = self.w.diffuse(self.dev)
        out[:d.shape[0]] = d
        return out

    def get_direct(self):
        if not self.traced:
            self.fail(capi.ERR_STATE, "rvb_get_direct: nothing traced")
        self.fetch_small()
        return self._of_pair("direct").copy()

    def get_image_candidates(self):
        if not self.traced:
            self.fail(capi.ERR_STATE, "rvb_get_image_candidates: nothing traced")
        self.fetch_small()
        return self.small_host["cand"].copy()

    # ---- kept.hip --------------------------------------------------------------------------------------------------------------------
    def keep_paths(self, on, listener=False):
        self.keep, self.keep_listener = bool(on), bool(on and listener)
        if not on and not self.forgot("keep_paths(0):release"):
            self.kept_valid = self.listener_valid = False

    def reshade_grad_map(self, predelay, sample_rate, nbins, device_weights_pointer, out=None):
        if not self.traced:
            self.fail(capi.ERR_STATE, "rvb_reshade_grad_map: nothing traced")
        if not (self.kept_valid and self.listener_valid):
            self.fail(capi.ERR_STATE, "rvb_reshade_grad_map: the last trace was made without RVB_KEEP_LISTENER")
        if not self.ir_configured:
            self.fail(capi.ERR_STATE, "rvb_reshade_grad_map: no IR configuration")
        if self.model[0] == "hrtf" or self.which != capi.IR_DIFFUSE or self.nchannels > 8:
            self.fail(capi.ERR_STATE, "rvb_reshade_grad_map: speakers, RVB_IR_DIFFUSE, 1 to 8 channels only")
        self.ensure_sort_buffers(self.dev.ndirs * self.dev.nrefl)
        self.sort_keys = "a gradient map's list"
        out.zero_()                                                       # (zero weights: every entry written, every entry 0)
        return out

    def reshade(self, surfaces, air):
        if not self.traced:
            self.fail(capi.ERR_STATE, "rvb_reshade: nothing traced")
        if not self.kept_valid:
            self.fail(capi.ERR_STATE, "rvb_reshade: the last trace was made without keeping")
        if surfaces is not None and surfaces.shape[0] != self.w.table(self.scene, "own").shape[0]:
            self.fail(capi.ERR_INVALID, "rvb_reshade: surface count")
        table = "own" if surfaces is None else next(t for t in cm.TABLES if self.w.table(self.scene, t) is surfaces)
        self.void_fetched_results("reshade:void_fetched_results")
        self.dev = self.kept_rec = self.kept_rec._replace(table=table, air=self._air(air), pattern=self.pattern)

    def relisten(self, mics):
        if not self.traced:
            self.fail(capi.ERR_STATE, "rvb_relisten: nothing traced")
        if not self.listener_valid:
            self.fail(capi.ERR_STATE, "rvb_relisten: the last trace was made without RVB_KEEP_LISTENER")
        if len(mics) != self.npairs:
            self.fail(capi.ERR_INVALID, "rvb_relisten: microphone count")
        self.void_fetched_results("relisten:void_fetched_results")
        self.dev = self.kept_rec = self.kept_rec._replace(mics=tuple(self._index("mics", m) for m in mics))

    # ---- sort.hip --------------------------------------------------------------------------------------------------------------------
    def ensure_sort_buffers(self, n):
        if n > self.sort_cap:
            self.sort_cap, self.sort_keys = n, "a fresh allocation"
        if not self.forgot("ensure_sort_buffers:tenant"):                 # on every call: whoever asks rewrites the buffers
            self.tenant = "nothing"

    # ---- flatten.hip -----------------------------------------------------------------------------------------------------------------
    def flatten_keys(self, array, sample_rate):
        self.ensure_sort_buffers(array.shape[0])                          # (in front of the upload into flat_in)
        self.sort_keys = ("flat", id(array), sample_rate)
        return self.w.oracle.flatten(array, sample_rate).shape[1]

    def flatten_query(self, array, sample_rate):
        bins = self.flatten_keys(array, sample_rate)
        self.tenant, self.query = "flatten query", (id(array), array.shape[0], sample_rate, bins)
        return bins

    def flatten_fill(self, array, sample_rate, capacity):
        resident = self.tenant == "flatten query" and self.query[:3] == (id(array), array.shape[0], sample_rate)
        bins = self.query[3] if resident else self.flatten_keys(array, sample_rate)
        if not self.forgot("flatten_fill:keys consumed"):
            self.tenant = "nothing"
        if capacity < bins:
            self.fail(capi.ERR_CAPACITY, "rvb_flatten: capacity_bins too small")
        # the ordered sum follows the keys that ARE in the sort buffers: another call's keys bin this array wrongly
        mine = self.sort_keys == ("flat", id(array), sample_rate)
        self.sort_keys = "consumed by the fill's sort"
        return self.w.oracle.flatten(array, sample_rate) if mine else np.zeros((8, bins), np.float32)

    def attenuate_speaker(self, mic, impulses, direction, coefficient):
        return self.w.oracle.attenuate_speaker(mic, impulses, direction, coefficient)

    def attenuate_hrtf(self, mic, impulses, table_channel, facing, up, channel):
        if not self.forgot("set_one_ear_table:hrtf_table_ears"):          # set_one_ear_table
            self.hrtf_table_ears = 1
        if not self.forgot("set_one_ear_table:drop_configuration"):
            self.drop_configuration()
        return self.w.oracle.attenuate_hrtf(mic, impulses, table_channel, facing, up, channel)

    # ---- ir.hip ----------------------------------------------------------------------------------------------------------------------
    def configure_common(self, kind, layout, which, images):
        if not self.traced:
            self.fail(capi.ERR_STATE, "rvb_ir_configure: nothing traced")
        self.images_host = np.array(images, dtype=IMPULSE)                # the context's own copy
        self.images_key = hash(self.images_host.tobytes())
        self.model, self.which, self.ir_configured = (kind, layout), which, True
        self.nchannels = 2 if kind == "hrtf" else len(cm.LAYOUTS[layout])
        if not self.forgot("configure_common:exact.valid"):
            self.void_exact_list()
        if not self.forgot("configure_common:range_pending"):
            self.range_pending = False

    def ir_configure_speakers(self, mic, directions, coefficients, which=capi.IR_ALL, images=None):
        layout = next(name for name, sp in cm.LAYOUTS.items() if [d for d, _ in sp] == list(directions) and [k for _, k in sp] == list(coefficients))
        self.configure_common("speakers", layout, which, images)

    def ir_configure_hrtf(self, mic, table, facing, up, which=capi.IR_ALL, images=None):
        if table is not None:
            self.hrtf_table = next(name for name in ("T", "U") if self.w.hrtf[name] is table)
            self.hrtf_table_ears = 2
        elif self.hrtf_table_ears != 2:
            self.fail(capi.ERR_STATE, "rvb_ir_configure_hrtf: table == NULL needs an earlier call with a table")
        self.configure_common("hrtf", self.hrtf_table, which, images)

    def channels(self):
        key = (self.dev, self.ir_pair, self.model, self.which, self.images_key)
        if key not in self._chans:
            if len(self._chans) > 32:
                self._chans.clear()
            parts = ([self._pair_diffuse()] if self.which & capi.IR_DIFFUSE else []) + ([self.images_host] if self.which & capi.IR_IMAGES else [])
            impulses = np.concatenate(parts) if parts else np.zeros(0, IMPULSE)
            mic = self.w.mic(self.dev.scene, self.dev.mics[self.ir_pair if self.ir_pair < len(self.dev.mics) else 0])
            self._chans[key] = self.w.attenuate_all(mic, impulses, *self.model)
        return self._chans[key]

    def ir_time_range_begin(self):
        if not self.ir_configured:
            self.fail(capi.ERR_STATE, "rvb_ir_time_range_begin: rvb_ir_configure_* first")
        if self.model[0] == "hrtf":
            self.range_host, self.range_pending = self.w.time_range(self.channels()), True

    def ir_time_range(self):
        if not self.ir_configured:
            self.fail(capi.ERR_STATE, "rvb_ir_time_range: rvb_ir_configure_* first")
        if self.model[0] == "hrtf":
            if not self.range_pending:
                self.range_host = self.w.time_range(self.channels())
            self.range_pending = False
            return self.range_host
        lo, hi = None, np.float32(0)
        if self.which & capi.IR_DIFFUSE:
            self.fetch_small()
            lo, hi = self._of_pair("range")
        if self.which & capi.IR_IMAGES:
            for im in self.images_host[(self.images_host["volume"] != 0).any(axis=1)]:
                if im["time"] != 0 and (lo is None or im["time"] < lo):
                    lo = im["time"]
                hi = max(hi, im["time"])
        return (float(lo) if lo is not None else 0.0), float(hi)

    def exact_prepare(self, predelay, sample_rate, nbins):
        chans = self.channels()
        self.ensure_sort_buffers(chans[0].shape[0] * (2 if self.model[0] == "hrtf" else 1))          # exact_begin
        self.sort_keys = "an exact list"
        self.tenant, self.exact = "exact list", {"nbins": nbins, "chans": chans, "predelay": predelay, "rate": sample_rate}

    def exact_fold(self, b0, b1, hist):
        e = self.exact
        self.w.accumulate(hist, e["chans"], e["predelay"], e["rate"], b0, b1)

    def ir_accumulate_tensor(self, predelay, sample_rate, nbins, mode, tensor):
        if not self.ir_configured:
            self.fail(capi.ERR_STATE, "rvb_ir_accumulate: rvb_ir_configure_* first")
        hist = tensor.numpy()
        assert hist.shape == (self.nchannels, 8, nbins)
        if mode == capi.IR_FAST and not (self.model[0] == "speakers" and self.nchannels > 8):
            self.w.accumulate(hist, self.channels(), predelay, sample_rate)        # (the atomic histogram: no sort buffers)
        else:
            self.exact_prepare(predelay, sample_rate, nbins)
            self.exact_fold(0, nbins, hist)
        if not self.forgot("accumulate:exact.valid"):
            self.void_exact_list()

    def ir_exact_prepare(self, predelay, sample_rate, nbins):
        if not self.ir_configured:
            self.fail(capi.ERR_STATE, "rvb_ir_exact_prepare: rvb_ir_configure_* first")
        self.exact_prepare(predelay, sample_rate, nbins)

    def ir_exact_fold_tensor(self, nbins, bin_begin, bin_end, tensor):
        if self.tenant != "exact list" or self.exact["nbins"] != nbins:
            self.fail(capi.ERR_STATE, "rvb_ir_exact_fold: rvb_ir_exact_prepare with this nbins first")
        hist = tensor.numpy()
        if hist.shape[0] != len(self.exact["chans"]):                   # (a list of another channel count: the fold would write other rows)
            hist[:] = np.float32(1.0)
            return
        self.exact_fold(bin_begin, bin_end, hist)

    def decay_curve_tensor(self, histogram, curve=None):
        return histogram.clone()                                          # (a block of its own: nothing of the context is touched)


@pytest.fixture(scope="module")
def world(oracle):
    return cm.World(oracle)


def walk(world, ops, forget=None, label="", **more):
    return Walk(world, LedgerContext(world, forget), "cpu", label, **more).run(ops)


def flagged(world, ops, forget):
    """(a stand-in that has forgotten something may also trip over its own state — an assertion, a lookup that finds nothing —: flagged too)"""
    assert forget is not None
    try:
        walk(world, ops, forget)
    except (Disagreement, AssertionError, StopIteration, LookupError, ValueError):
        return True
    return False


WALKS = [("directed", name) for name in cm.DIRECTED] + [("seed", seed) for seed in cm.SEEDS]


def ops_of(kind, name):
    return cm.DIRECTED[name] if kind == "directed" else cm.seeded_walk(name)


@pytest.fixture(scope="module")
def complete(world):
    """every walk on the complete stand-in: it must agree with the model; the walks are kept for the coverage conditions"""
    return {(kind, name): walk(world, ops_of(kind, name), None, "%s %s" % (kind, name), keep_histograms=kind == "directed" and "on_top" in name)
            for kind, name in WALKS}


def test_the_grounds_of_the_menus(world):
    """No walk may pass on empty ground: every pair of the menus sees its source, has image sources, live and silent records, and the
    other table, the other air, the other microphone and the pattern each change the records and the time range."""
    for scene in cm.SCENES:
        for mic in (0, 1):
            for source in (0, 1):
                a = world.trace(scene, "own", "A", mic, source, 130, 24, False)
                assert (a["direct"]["volume"] != 0).any(), (scene, mic, source)
                if (mic, source) == cm.PAIRS[0]:                  # (the pair of the directed sequences and of every checkpoint's first trace)
                    assert a["merged"].shape[0] >= 2 and a["cand"].shape[0] >= 1, (scene, mic, source)
                live = (a["diffuse"]["volume"] != 0).any(axis=1)
                assert live.any(), (scene, mic, source)
                for other in (world.trace(scene, "B", "A", mic, source, 130, 24, False), world.trace(scene, "own", "B", mic, source, 130, 24, False),
                              world.trace(scene, "own", "A", 1 - mic, source, 130, 24, False), world.trace(scene, "own", "A", mic, source, 130, 24, True)):
                    assert not cm.same_records(other["diffuse"], a["diffuse"])         # (the direct slot does not depend on the table)
    hall = world.trace("cathedral", "own", "A", 0, 0, 509, 24, False)
    muted = world.trace("cathedral", "B", "B", 0, 0, 509, 24, False)
    rng = lambda r: world.time_range([world.oracle.attenuate_speaker((0, 0, 0), r["diffuse"], (0, 0, 1), 0.0)])
    assert rng(hall) != rng(muted), "the table that mutes a surface does not move the range"
    assert not (~(hall["diffuse"]["volume"] != 0).any(axis=1)).all()


def test_the_serial_sum_of_the_model_is_the_oracles_flatten(world):
    """The model continues a histogram with serial_add; on a zeroed histogram that must be oracle.flatten itself, bit for bit."""
    for name, rate in (("edge", 8192.0), ("edge", 44100.0), ("big", 44100.0)):
        att = world.flat_array(name)
        want = world.oracle.flatten(att, rate)
        got = np.zeros_like(want)
        cm.serial_add(got, cm.time_bins(att["time"], rate), att["volume"])
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, rate)
        assert cm.ir_bins(float(att["time"].max()), 0.0, rate) == want.shape[1]


def test_the_model_and_the_complete_stand_in_agree_on_every_walk(complete):
    assert len(complete) == len(cm.DIRECTED) + len(cm.SEEDS)


@pytest.mark.parametrize("forget", FORGETS)
def test_a_forgotten_invalidation_is_flagged(world, complete, forget):
    directed = next((name for name in cm.DIRECTED if flagged(world, cm.DIRECTED[name], forget)), None)
    assert directed, "no directed sequence notices " + forget
    seeds = []
    for seed in cm.SEEDS:                       # (a flagged walk ends where it is flagged; the count stops at the quarter asked for)
        if 4 * len(seeds) < len(cm.SEEDS) and flagged(world, cm.seeded_walk(seed), forget):
            seeds.append(seed)
    print("%s: flagged by the directed sequence %s and by the seeds %s" % (forget, directed, seeds))
    assert 4 * len(seeds) >= len(cm.SEEDS), "only seeds %s notice %s" % (seeds, forget)


OPERATIONS = ("set_scene", "set_directions", "keep_paths", "set_source_pattern", "trace", "trace_pairs", "select_pair", "reshade", "relisten",
              "configure_speakers", "configure_hrtf", "time_range_begin", "time_range", "accumulate", "prepare", "fold", "flatten_query",
              "flatten_fill", "attenuate_speaker", "attenuate_hrtf", "get_raw_diffuse", "get_direct", "get_image_candidates", "decay_curve", "grad_map")
REFUSALS = (("trace", capi.ERR_STATE), ("select_pair", capi.ERR_STATE), ("select_pair", capi.ERR_INVALID), ("reshade", capi.ERR_STATE),
            ("reshade", capi.ERR_INVALID), ("relisten", capi.ERR_STATE), ("relisten", capi.ERR_INVALID), ("get_raw_diffuse", capi.ERR_STATE),
            ("get_direct", capi.ERR_STATE), ("get_image_candidates", capi.ERR_STATE), ("configure_speakers", capi.ERR_STATE),
            ("configure_hrtf", capi.ERR_STATE), ("time_range_begin", capi.ERR_STATE), ("time_range", capi.ERR_STATE),
            ("accumulate", capi.ERR_STATE), ("prepare", capi.ERR_STATE), ("fold", capi.ERR_STATE), ("grad_map", capi.ERR_STATE))


def grows_after_a_shrink(sizes):
    """some a > b < c in order"""
    return any(sizes[i] > sizes[j] and any(c > sizes[j] for c in sizes[j + 1:]) for i in range(len(sizes)) for j in range(i + 1, len(sizes)))


def test_what_the_seeds_cover(complete):
    seen = collections.Counter()
    for seed in cm.SEEDS:
        w = complete["seed", seed]
        seen.update(w.seen)
        records = [e[1] for e in w.events if e[0] == "records"]
        modes = [e[2] for e in w.events if e[0] == "records"]
        images = [e[1] for e in w.events if e[0] == "images"]
        kinds = [e[2] for e in w.events if e[0] == "images"]
        keys = [e[1] for e in w.events if e[0] == "keys"]
        switches = {(a, b) for a, b in zip(modes, modes[1:]) if a != b}
        print("seed %d: %d operations; %d traces, %d configurations, %d sorted lists; refusals %d"
              % (seed, len(w.ops), len(records), len(images), len(keys), sum(n for k, n in w.seen.items() if isinstance(k, tuple) and k[0] not in ("exact", "fast"))))
        assert w.seen["on top"] >= 1, (seed, "no EXACT accumulate really went on top of a histogram of more than one bin")
        assert grows_after_a_shrink(records) and grows_after_a_shrink(images) and grows_after_a_shrink(keys), seed
        assert switches == {(True, False), (False, True)}, (seed, "key-mode switches of the trace")
        changes = [k for k, prev in zip(kinds, [None] + kinds) if k != prev]
        assert any(changes[i:i + 3] == ["speakers", "hrtf", "speakers"] for i in range(len(changes))), seed
    for op in OPERATIONS:
        assert seen[op], op
    for refusal in REFUSALS:
        assert seen[refusal], refusal
    for cls in cm.NBINS:
        assert seen["exact", cls] + seen["fast", cls], cls              # (each class in each mode: the directed nbins_classes_* sequences)
    print("over all seeds:", {str(k): n for k, n in sorted(seen.items(), key=str)})


def test_the_directed_sequences_hold_what_their_names_say(complete):
    """every nbins class in the five model / mode combinations, and the refusals of the directed state sequences"""
    for name in cm.DIRECTED:
        if name.startswith("nbins_classes"):
            mode = "fast" if name.endswith("fast") else "exact"
            assert all(complete["directed", name].seen[mode, cls] == 1 for cls in cm.NBINS), name
    assert cm.on_top_is_the_all_chain(complete["directed", "diffuse_then_images_on_top_is_the_all_chain"])
    seen = complete["directed", "calls_before_a_scene_are_refused"].seen
    assert seen["trace"] == 1 and all(seen[op, capi.ERR_STATE] == 1 for op in (
        "trace", "trace_pairs", "get_raw_diffuse", "get_direct", "get_image_candidates", "select_pair", "configure_speakers", "configure_hrtf", "time_range_begin",
        "time_range", "accumulate", "prepare", "fold", "reshade", "relisten"))
    seen = complete["directed", "the_gradient_map_uses_the_sort_buffers"].seen
    assert seen["grad_map"] == 2 and seen["grad_map", capi.ERR_STATE] == 6 and seen["fold", capi.ERR_STATE] == 1 and seen["time_range"] == 1
    seen = complete["directed", "prepare_then_decay_curve_flatten_attenuate"].seen
    assert seen["fold"] == 4 and seen["fold", capi.ERR_STATE] == 5
    seen = complete["directed", "hrtf_table_after_a_one_ear_attenuate"].seen
    assert seen["configure_hrtf", capi.ERR_STATE] == 2 and seen["configure_hrtf"] == 3
    seen = complete["directed", "keeping_switched_on_after_the_trace"].seen
    assert seen["reshade", capi.ERR_STATE] >= 3 and seen["reshade"] >= 2 and seen["relisten", capi.ERR_INVALID] == 1
