"""the post-processing chain and the drop-in CLI surface.

* the reference's own cmd/main.cpp must compile and link UNCHANGED against include/rayverb +
  include/shims + librayverb.so (build() does that into oracle/_ref/ where the reference checkout is
  present, oracle/ref/build_ref.sh; its demo inputs are fixtures under tests/golden/assets);
* process() / RayverbFiltering against an independent numpy/scipy restatement of reference
  rayverb/filters.cpp + rayverb.cpp:79-149 (the reference has no tests or fixtures for these:
  parity unpinned, SURVEY §8(c) gap 3 — the restatement below is the stated algorithm);
* on the GPU: config -> trace -> attenuate -> predelay -> flatten -> process -> sound file."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT

PKG = os.path.join(ROOT, "parallel-reverb-raytracer_amd")
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
ASSETS = os.path.join(ROOT, "tests", "golden", "assets")
REFERENCE_CLI = os.path.join(ROOT, "oracle", "_ref", "parallel_raytrace")
REFERENCE_CLI_DIAG = os.path.join(ROOT, "oracle", "_ref", "parallel_raytrace_diag")
NOT_BUILT = "oracle/_ref/parallel_raytrace not built (build() compiles it where the reference checkout is present)"
INC = ["-I" + os.path.join(ROOT, "include", "rayverb"), "-I" + os.path.join(ROOT, "include", "shims"), "-I" + os.path.join(ROOT, "include")]
LINK = ["-L" + PKG, "-lrayverb", "-lrvb_hip", "-Wl,-rpath," + PKG]


def _compile(src, out, std="-std=c++11", extra=()):
    subprocess.check_call(["make", "-C", PKG, "-j4"], stdout=subprocess.DEVNULL)
    os.makedirs(BUILD, exist_ok=True)
    subprocess.check_call(["g++", std, "-O1", "-w"] + list(extra) + INC + [src, "-o", out] + LINK)
    return out


@pytest.mark.skipif(not os.path.exists(REFERENCE_CLI), reason=NOT_BUILT)
def test_reference_cli_compiles_unchanged_and_fails_like_the_reference_without_gpu(tmp_path):
    import torch
    args = [REFERENCE_CLI, os.path.join(ASSETS, "near_c.json"), os.path.join(ASSETS, "echo_tunnel.obj"), os.path.join(ASSETS, "mat.json"),
            str(tmp_path / "o.aif")]
    if not torch.cuda.is_available():
        r = subprocess.run(args, capture_output=True, text=True)
        assert r.returncode == 1 and "encountered opencl error" in r.stderr and "no CPU path" in r.stderr
    # a demo config the reference itself rejects ("hipass": false is not a number, config.h:143-146)
    args[1] = os.path.join(ASSETS, "tunnel.json")
    r = subprocess.run(args, capture_output=True, text=True)
    assert r.returncode == 1 and "invalid value" in r.stderr


@pytest.mark.skipif(not os.path.exists(REFERENCE_CLI), reason=NOT_BUILT)
def test_reference_cli_diagnostic_build_links(tmp_path):
    """-DDIAGNOSTIC makes cmd/main.cpp:270-278 call print_diagnostic (the impulse.dump writer, helpers.cpp:19-59)."""
    assert os.path.exists(REFERENCE_CLI_DIAG)


# ---- independent restatement of the post-processing chain ---------------------------------------------
EDGES = [175, 350, 700, 1400, 2800, 5600, 11200, 20000]


def _biquad(x, b0, b1, b2, a1, a2):
    from scipy.signal import lfilter
    return lfilter([b0, b1, b2], [1.0, a1, a2], x.astype(np.float64)).astype(np.float32)


def _twopass(x, *c):
    return _biquad(_biquad(x, *c)[::-1], *c)[::-1]


def _bandpass_coeffs(lo, hi, sr):
    lo, hi, sr = np.float32(lo), np.float32(hi), np.float32(sr)
    c = np.sqrt(np.float64(lo * hi))
    omega = 2 * np.pi * c / np.float64(sr)
    cs, sn = np.cos(omega), np.sin(omega)
    q = sn / (np.log(2) * np.log2(np.float64(hi / lo)) * omega)
    alpha = sn * np.sinh(1 / (2 * q))
    n = 1 / (1 + alpha)
    return n * alpha, 0.0, -n * alpha, n * -2 * cs, n * (1 - alpha)


def _lr_coeffs(lo, hi, sr):
    def getc(co):
        w = np.pi * np.float64(np.float32(co)) / np.float64(np.float32(sr))
        return np.cos(w) / np.sin(w)
    c = getc(hi); a0 = c * c + c * np.sqrt(2) + 1
    lop = (1 / a0, 2 / a0, 1 / a0, -2 * (c * c - 1) / a0, (c * c - c * np.sqrt(2) + 1) / a0)
    c = getc(lo); a0 = c * c + c * np.sqrt(2) + 1
    hip = (c * c / a0, -2 * c * c / a0, c * c / a0, -2 * (c * c - 1) / a0, (c * c - c * np.sqrt(2) + 1) / a0)
    return lop, hip


def _sinc_kernel(lo, hi, sr):
    def lopass(cut, length):
        i = np.arange(length)
        off = i / (length - 1.0)
        win = (7938 / 18608.0 - 9240 / 18608.0 * np.cos(2 * np.pi * off) + 1430 / 18608.0 * np.cos(4 * np.pi * off)).astype(np.float32)
        t = 2 * np.float64(np.float32(cut) / np.float32(sr)) * (i - (length - 1) / 2.0)
        with np.errstate(invalid="ignore", divide="ignore"):
            k = np.where(i == (length - 1) // 2, 1.0, np.sin(np.pi * t) / (np.pi * t)).astype(np.float32)
        k = (win * k).astype(np.float32)
        return (k * np.float32(1.0 / np.abs(k).max())).astype(np.float32)
    lop = lopass(hi, 15)
    hip = -lopass(lo, 15)
    hip[7] += 1
    return (np.convolve(lop.astype(np.float64), hip.astype(np.float64)) * 29).astype(np.float32)


def _process(data, ft, sr, do_normalize, lo_cutoff, do_trim, scale):
    out = []
    for ch in data:
        bands = []
        for b in range(8):
            lo, hi = ([lo_cutoff] + EDGES)[b], EDGES[b]
            x = ch[b]
            if ft == 0:
                k = _sinc_kernel(lo, hi, sr)
                n = len(k) + len(x) - 1
                x = (np.convolve(k.astype(np.float64), x.astype(np.float64)) * n).astype(np.float32)
            elif ft == 1:
                x = _biquad(x, *_bandpass_coeffs(lo, hi, sr))
            elif ft == 2:
                x = _twopass(x, *_bandpass_coeffs(lo, hi, sr))
            else:
                lop, hip = _lr_coeffs(lo, hi, sr)
                x = _twopass(_twopass(x, *lop), *hip)
            bands.append(x)
        mix = np.zeros(len(bands[0]), np.float32)
        for x in bands:
            mix = (mix + x).astype(np.float32)
        out.append(mix)
    if do_normalize:
        f = np.float32(1.0 / max(np.abs(c).max() for c in out))
        out = [(c * f).astype(np.float32) for c in out]
    if scale != 1:
        out = [(c * np.float32(scale)).astype(np.float32) for c in out]
    if do_trim:
        last = max(int(np.nonzero(np.abs(c) >= np.float32(0.00001))[0].max()) if (np.abs(c) >= np.float32(0.00001)).any() else -1 for c in out)
        out = [c[:max(last, 0)] for c in out]     # the last audible sample itself is dropped (quirk Q8)
    return out


@pytest.mark.parametrize("ft", [0, 1, 2, 3])
def test_process_matches_independent_restatement(tmp_path, ft):
    tool = _compile(os.path.join(ROOT, "tests", "cpp", "postprocess_tool.cpp"), os.path.join(BUILD, "postprocess_tool"))
    rng = np.random.default_rng(ft)
    channels, n = 2, 3000
    data = np.zeros((channels, 8, n), np.float32)
    idx = rng.integers(0, n - 500, (channels, 8, 200))
    for c in range(channels):
        for b in range(8):
            np.add.at(data[c, b], idx[c, b], rng.uniform(-1, 1, 200).astype(np.float32) * np.exp(-idx[c, b] / 400.0).astype(np.float32))
    (tmp_path / "in.bin").write_bytes(data.tobytes())
    subprocess.check_call([tool, str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), str(channels), str(n), str(ft), "44100", "1", "45", "1", "0.5"])
    raw = (tmp_path / "out.bin").read_bytes()
    got, off = [], 0
    for _ in range(channels):
        m = struct.unpack_from("q", raw, off)[0]; off += 8
        got.append(np.frombuffer(raw, np.float32, m, off)); off += 4 * m
    want = _process(data, ft, 44100.0, True, 45.0, True, 0.5)
    for g, w in zip(got, want):
        assert abs(len(g) - len(w)) <= 1          # a sample sitting exactly at the trim threshold may differ
        k = min(len(g), len(w))
        assert k > 100 and np.abs(g[:k] - w[:k]).max() <= 2e-5 * 0.5


@pytest.mark.gpu
def test_cli_flow_end_to_end(tmp_path):
    exe = _compile(os.path.join(ROOT, "tests", "cpp", "cli_flow.cpp"), os.path.join(BUILD, "cli_flow"))
    assets = os.path.join(ROOT, "tests", "golden", "assets")
    for name, model in (("speakers", {"speakers": [{"direction": [-1, 0, -1], "shape": 0.5}, {"direction": [1, 0, -1], "shape": 0.5}]}),
                        ("hrtf", {"hrtf": {"facing": [0, 0, 1], "up": [0, 1, 0]}})):
        cfg = {"rays": 4096, "reflections": 32, "sample_rate": 44100, "bit_depth": 16, "source_position": [0, 2, 2], "mic_position": [0, 2, 0],
               "attenuation_model": model, "filter": "linkwitz_riley", "trim_predelay": True, "output_mode": "all", "hipass": 60}
        (tmp_path / (name + ".json")).write_text(json.dumps(cfg))
        out = tmp_path / (name + ".wav")
        r = subprocess.run([exe, str(tmp_path / (name + ".json")), os.path.join(assets, "large_square.obj"), os.path.join(assets, "mat.json"), str(out)],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        raw = out.read_bytes()
        assert raw[:4] == b"RIFF" and raw[8:12] == b"WAVE" and struct.unpack_from("<H", raw, 22)[0] == 2
        pcm = np.frombuffer(raw[44:], dtype="<i2").reshape(-1, 2)
        assert pcm.shape[0] > 1000 and np.abs(pcm).max() >= 32000      # normalised to full scale
