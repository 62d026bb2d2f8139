"""TEST INFRASTRUCTURE: a stand-in with the method surface of capi.Context whose compute is the CPU
oracle.  It lets the multi-process orchestration of parallel_reverb_raytracer_amd.distributed run
under gloo on machines without a GPU.  Never used by the product."""
import numpy as np

from parallel_reverb_raytracer_amd import capi
from parallel_reverb_raytracer_amd.dtypes import ATTENUATED, IMPULSE, NUM_IMAGE_SOURCE


class OracleTracer:
    def __init__(self, oracle, scene, directions):
        self.oracle, self.scene, self.directions = oracle, scene, directions
        self.nchannels = 0
        self.nrays = int(directions.shape[0])

    def set_concurrent_traces(self, traces):
        pass                                                           # (a sizing hint for the path kernel)

    def trace(self, mic, source, nreflections, air, ray_offset=0):
        self._trace(((mic, source),), nreflections, air, ray_offset)

    @staticmethod
    def trace_group(tracers, mics, sources, nreflections, air, ray_offsets=None):
        for k, t in enumerate(tracers):
            t.trace(mics[k], sources[k], nreflections, air, ray_offsets[k] if ray_offsets is not None else 0)

    def trace_pairs(self, mics, sources, nreflections, air, ray_offset=0):
        """One oracle run per pair; select_pair(k) picks the pair the ir_* calls and get_direct work on (pair 0 to begin with)."""
        self._trace(tuple(zip(mics, sources)), nreflections, air, ray_offset)

    def _trace(self, pairs, nreflections, air, ray_offset):
        self.pairs = [(mic, self.oracle.raytrace(self.scene, mic, source, self.directions, nreflections, air)) for mic, source in pairs]
        self.ray_offset = ray_offset
        self.mic, (self.diffuse, self.image, self.index) = self.pairs[0]

    def select_pair(self, pair):
        self.mic, (self.diffuse, self.image, self.index) = self.pairs[pair]

    def get_image_candidates(self):
        """All pairs' candidates, ray numbers global: ray + pair * nrays (+ the trace's ray_offset)."""
        parts = []
        for pair, (_, (_, image, index)) in enumerate(self.pairs):
            idx = index.reshape(self.nrays, NUM_IMAGE_SOURCE)
            rays, slots = np.nonzero(idx[:, 1:])
            cand = np.zeros(rays.shape[0], dtype=capi.IMAGE_CANDIDATE)
            cand["ray"], cand["slot"] = rays + pair * self.nrays + self.ray_offset, slots + 1
            cand["index"] = idx[rays, slots + 1]
            cand["impulse"] = image.reshape(self.nrays, NUM_IMAGE_SOURCE)[rays, slots + 1]
            parts.append(cand)
        return np.concatenate(parts)

    get_pair_candidates = capi.Context.get_pair_candidates             # (pure host code over get_image_candidates and nrays)

    def get_direct(self):
        return self.image[:1].copy()

    def ir_configure_speakers(self, mic, directions, coefficients, which, images):
        parts = []
        if which & capi.IR_DIFFUSE:
            parts.append(self.diffuse)
        if which & capi.IR_IMAGES:
            parts.append(np.ascontiguousarray(images, dtype=IMPULSE))
        self.impulses = np.concatenate(parts) if parts else np.zeros(0, IMPULSE)
        self.channels = [self.oracle.attenuate_speaker(mic, self.impulses, d, c) for d, c in zip(directions, coefficients)]
        self.nchannels = len(self.channels)

    def ir_configure_hrtf(self, mic, table, facing, up, which=capi.IR_ALL, images=None):
        parts = []
        if which & capi.IR_DIFFUSE:
            parts.append(self.diffuse)
        if (which & capi.IR_IMAGES) and images is not None:
            parts.append(np.ascontiguousarray(images, dtype=IMPULSE))
        self.impulses = np.concatenate(parts) if parts else np.zeros(0, IMPULSE)
        self.channels = [self.oracle.attenuate_hrtf(mic, self.impulses, table[ch], facing, up, ch) for ch in (0, 1)]
        self.nchannels = 2

    def ir_time_range(self):
        t = np.concatenate([c["time"] for c in self.channels]) if self.channels else np.zeros(0, np.float32)
        nz = t[t != 0]
        return (float(nz.min()) if nz.size else 0.0), (float(t.max()) if t.size else 0.0)

    def ir_bins(self, max_time, predelay, sample_rate):
        t = np.float32(max_time) - np.float32(predelay) if max_time > predelay else np.float32(0)
        return int(np.round(np.float32(t * np.float32(sample_rate))) + 1)

    def ir_accumulate_tensor(self, predelay, sample_rate, nbins, mode, tensor):
        """Continues the reference's serial float sum (rayverb.cpp:67-74) ON TOP of what the histogram holds, impulse by impulse, as
        rvb_ir_accumulate does in exact mode (on a zeroed histogram that is flattenImpulses itself)."""
        for ch, att in enumerate(self.channels):
            att = att.copy()
            self.oracle.fix_predelay(att, predelay)
            hist = tensor[ch].numpy()                                  # shares the tensor's memory
            x = att["time"] * np.float32(sample_rate)                  # rayverb.cpp:69 round(): half away from zero (x >= 0; x - floor(x) is exact)
            f = np.floor(x)
            bins = np.where(x - f >= np.float32(0.5), f + 1, f).astype(np.int64)
            vol = att["volume"]
            for i in range(att.shape[0]):
                hist[:, bins[i]] += vol[i]

    def ir_accumulate_wait_for_torch(self):
        pass                                                           # (one host thread, no streams: everything is in program order)

    def export_tensor_to_host(self, tensor, host):
        host.copy_(tensor)

    def ir_accumulate_export_tensor(self, predelay, sample_rate, nbins, mode, tensor, host, slices=0):
        OracleTracer.ir_accumulate_tensor(self, predelay, sample_rate, nbins, mode, tensor)
        host.copy_(tensor)

    def synchronize_exports(self):
        pass

    def ir_exact_prepare(self, predelay, sample_rate, nbins):
        """The per-impulse bins of every channel (what rvb_ir_exact_prepare sorts on the GPU)."""
        self._prepared = []
        for att in self.channels:
            att = att.copy()
            self.oracle.fix_predelay(att, predelay)
            x = att["time"] * np.float32(sample_rate)
            f = np.floor(x)
            self._prepared.append((np.where(x - f >= np.float32(0.5), f + 1, f).astype(np.int64), att["volume"]))

    def ir_exact_fold_tensor(self, nbins, bin_begin, bin_end, tensor):
        """Bins [bin_begin, bin_end): every bin's impulses in impulse order on top of what the histogram holds."""
        for ch, (bins, vol) in enumerate(self._prepared):
            hist = tensor[ch].numpy()
            for i in np.nonzero((bins >= bin_begin) & (bins < bin_end))[0]:
                hist[:, bins[i]] += vol[i]

    def synchronize(self):
        pass
