"""The echo finder: which paths carry the energy of a time window of a finished trace (include/rvb_capi_window.h).

A reflectogram shows a peak — a slap at 180 ms, a flutter, a late cluster in one band — and the question is through which sequence of
walls that sound travelled.  `strongest_paths` asks the device for the strongest diffuse records behind the window and the hit points
of their rays; `polyline` turns one of them into the vertices to draw in the model.  The records are read as they stand: after a
reshade or a relisten the answer is that of the new materials or the new microphone.  Image sources and the direct sound are not
listed in this version."""
import numpy as np


def strongest_paths(ctx, t_begin, t_end, weights=None, max_paths=64, max_hits=None):
    """(paths, hits, in_window) of capi.Context.window_paths for the selected pair of `ctx`, whose last trace was kept with
    keep_paths(True, listener=True).  weights: eight band weights of the score sum_b (weights[b] * volume[b])^2, None = ones — one
    band alone with a unit vector.  max_hits defaults to the trace's nreflections: every path whole."""
    if max_hits is None:
        max_hits = ctx.nreflections
    return ctx.window_paths(t_begin, t_end, weights=weights, max_paths=max_paths, max_hits=max_hits)


def polyline(paths, hits, i, source, mic):
    """The vertices of path i for drawing, float32 [stored hits + 2][3]: the source, the hits the call stored for the path, the microphone."""
    stored = min(int(paths["nhits"][i]), hits.shape[1])
    out = np.empty((stored + 2, 3), dtype=np.float32)
    out[0] = np.asarray(source, dtype=np.float32).reshape(3)
    out[1:-1] = hits["position"][i, :stored]
    out[-1] = np.asarray(mic, dtype=np.float32).reshape(3)
    return out
