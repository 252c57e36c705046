"""include/pirip_hip.h section P (the band monitor) without a GPU: the library, the header, the binding and the CLI are there; the host
helpers (window, bin(f), nrows, db, occupied) are the statement's; and the inputs of tests/test_spectrum.py reach what they claim on the
statement alone (tests/specref.py): nothing near a denormal or an overflow decides an equality, the occupied bands stand 10 dB above the
empty one, and the on-bin tone peaks in its bin."""
import inspect
import json
import os
import re

import numpy as np
import pytest

import specref
import specshapes as sh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPEC_SYMBOLS = ("pirip_hip_spec_create", "pirip_hip_spec_destroy", "pirip_hip_spec_get_info", "pirip_hip_spec_window", "pirip_hip_spec_band_bins",
                "pirip_hip_spec_nrows", "pirip_hip_spec_push", "pirip_hip_spec_reset")
DASH_KEYS = set(json.load(open(os.path.join(ROOT, "tests", "golden", "dash_keys.json"))))


def test_library_header_binding_and_cli(built_lib):
    import pirip_amd
    hdr = open(os.path.join(ROOT, "include", "pirip_hip.h")).read()
    assert "section P" in hdr and "#define PIRIP_HIP_ABI_VERSION 2" in hdr
    for n in SPEC_SYMBOLS:
        assert hasattr(built_lib, n) and n + "(" in hdr, n
    sig = inspect.signature(pirip_amd.HipSpectrum)
    assert list(sig.parameters)[:2] == ["Fs", "nfft"]
    for k, v in (("hop", None), ("avg", 1), ("nstreams", 1), ("bands", ()), ("in_format", pirip_amd.IN_CU8_CSDR)):
        assert sig.parameters[k].default == v, k
    for m in ("window", "band_bins", "nrows", "push", "reset", "db", "occupied"):
        assert callable(getattr(pirip_amd.HipSpectrum, m)), m
    assert (pirip_amd.IN_CU8_CSDR, pirip_amd.IN_CF32) == (specref.U8, specref.CF32)
    assert pirip_amd.SPEC_BAND_ROW_DTYPE == specref.BAND_ROW
    assert os.access(os.path.join(ROOT, "pirip_amd", "bin", "iq_spectrum"), os.X_OK)


@pytest.mark.parametrize("nfft", specref.NFFTS)
def test_window_is_the_formula(built_lib, nfft):
    import pirip_amd
    w = pirip_amd.spec_window(nfft)
    f = (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(nfft) / nfft)).astype(np.float32)
    ulp = np.spacing(np.maximum(np.abs(f), np.float32(2.0 ** -126)))
    assert np.all(np.abs(w.astype(np.float64) - f.astype(np.float64)) <= ulp)
    assert w[0] == 0.0 and w[nfft // 2] == 1.0
    assert np.array_equal(w[1:], w[1:][::-1])                       # w[i] == w[nfft - i]
    assert np.array_equal(w.view(np.uint32), specref.window(nfft).view(np.uint32))
    assert built_lib.pirip_hip_spec_window(nfft, None) == -1 and built_lib.pirip_hip_spec_window(512, w.ctypes.data) == -6


def test_bin_of_at_the_edges_and_the_half_bin_boundaries():
    Fs = sh.FS
    for nfft in specref.NFFTS:
        b = lambda f: specref.bin_of(f, nfft, Fs)
        assert b(-Fs // 2) == nfft // 2 and b(0) == 0 and b(-1) == 0 and b(Fs // 2 - 1) == nfft // 2       # 1 Hz is well inside half a bin
        assert specref.band_bins(*sh.bands(nfft)[sh.BAND["all"]][1:], nfft, Fs) == (nfft // 2, nfft)
        # the boundary between bins k and k + 1 is (k + 1/2) Fs / nfft: the largest integer below it is bin k, the smallest at or above it k + 1
        for k in (0, 1, nfft // 8, nfft // 2 - 2, -1, -2, -nfft // 2):
            edge2 = (2 * k + 1) * Fs                                    # 2 nfft times the boundary
            below, above = (edge2 - 1) // (2 * nfft), -((-edge2) // (2 * nfft))
            assert b(below) == k % nfft and b(above) == (k + 1) % nfft, (nfft, k)
    # a small case by hand: Fs = 8, nfft = 4, bins at 0, 2, -4 (= 4), -2 Hz
    assert [specref.bin_of(f, 4, 8) for f in (-4, -3, -2, -1, 0, 1, 2, 3)] == [2, 3, 3, 0, 0, 1, 1, 2]
    assert specref.band_bins(-2, 1, 4, 8) == (3, 3) and specref.band_bins(3, 3, 4, 8) == (2, 1)


def _brute_rows(t, nfft, hop, avg):
    k = 0
    while k * hop + nfft <= t:
        k += 1
    return k // avg


@pytest.mark.parametrize("nfft,hop,avg", sorted({(c[0], c[1], c[3]) for c in sh.CASES}))
def test_nrows_against_a_brute_force_count(nfft, hop, avg):
    n = sh.length(nfft, hop, avg)
    # (the cutting test runs the cases with avg = 3: two of their rows are longer than its 2 nfft + 3 single samples)
    for cut in [sh.two_calls(n)] + (sh.cuttings(nfft, hop, avg, n) if avg == sh.CUT_AVG else []):
        assert sum(cut) == n and min(cut) >= 1
        pos = 0
        for c in cut:
            assert specref.nrows(pos, c, nfft, hop, avg) == _brute_rows(pos + c, nfft, hop, avg) - _brute_rows(pos, nfft, hop, avg)
            pos += c
    assert _brute_rows(n, nfft, hop, avg) == 2
    if avg == sh.CUT_AVG:
        third = sh.cuttings(nfft, hop, avg, n)[2]
        assert specref.nrows(0, third[0], nfft, hop, avg) == 0 and specref.nrows(third[0], 1, nfft, hop, avg) == 1


@pytest.mark.parametrize("nfft,hop,fmt,avg", sh.CASES)
def test_inputs_stay_clear_of_denormals_and_overflow(nfft, hop, fmt, avg):
    x = sh.inputs(nfft, hop, fmt, avg)
    w = specref.window(nfft)
    if fmt == "u8":
        assert x[1].min() == 0 and x[1].max() == 255
    else:
        assert abs(np.mean(x[1])) > 0.1                                 # the DC offset
    lo, hi = 2.0 ** -100, 2.0 ** 100
    for r in range(sh.NSTREAMS):
        z = specref.to_float(x[r], sh.FMT[fmt])
        for k in range(specref.segments(len(z), nfft, hop)):
            for part in specref.segment_parts(z, k, nfft, hop, w):
                a = np.abs(np.ascontiguousarray(part).view(np.float32).astype(np.float64))
                nz = a[a != 0]
                assert nz.min() >= lo and nz.max() < hi, (r, k)


@pytest.mark.parametrize("nfft,hop,fmt,avg", sh.CASES)
def test_bands_show_what_they_claim(built_lib, nfft, hop, fmt, avg):
    import pirip_amd
    rws, bnd = sh.expected(nfft, hop, fmt, avg)
    assert rws.shape == (3, 2, nfft) and bnd.shape == (len(sh.bands(nfft)), 2)
    nbins = [specref.band_bins(lo, hi, nfft, sh.FS)[1] for _, lo, hi in sh.bands(nfft)]
    per_bin = bnd["power"].astype(np.float64) / np.array(nbins)[:, None]
    for q in sh.BAND["chan"]:
        assert np.all(10 * np.log10(per_bin[q] / per_bin[sh.BAND["empty"]]) >= 10.0), q
    assert nbins[sh.BAND["one"]] == 1 and nbins[sh.BAND["all"]] == nfft
    first, count = specref.band_bins(*sh.bands(nfft)[sh.BAND["wrap"]][1:], nfft, sh.FS)
    assert first + count > nfft                                         # walks across bin 0
    for q in (sh.BAND["one"],) + sh.BAND["overlap"]:
        assert np.all(bnd["peak_bin"][q] == sh.on_bin(nfft)), q
    # one bin: its power is its peak is the row's value
    assert np.array_equal(bnd["power"][sh.BAND["one"]], rws[0][:, sh.on_bin(nfft)]) and np.array_equal(bnd["peak"][sh.BAND["one"]], bnd["power"][sh.BAND["one"]])
    # db and occupied, the binding's host helpers against the statement's
    scl = specref.scale(nfft, avg)
    d = pirip_amd.spec_db(rws, scl)
    assert np.array_equal(d, specref.db(rws, scl)) and d.shape == rws.shape
    assert np.all(np.argmax(d[0], axis=-1) == sh.on_bin(nfft) + nfft // 2)          # on dash.py's axis the tone sits at 30 kHz
    occ = pirip_amd.spec_occupied(bnd, nbins, sh.BAND["empty"], 10.0)
    assert occ.shape == (len(nbins), 2)
    assert all(occ[q].all() for q in sh.BAND["chan"]) and not occ[sh.BAND["empty"]].any()
    assert np.array_equal(occ, per_bin > per_bin[sh.BAND["empty"]][None, :] * 10.0)


def test_dash_line_has_the_keys_dash_py_reads():
    src = open(os.path.join(ROOT, "pirip_amd", "tools", "iq_spectrum.cpp")).read()
    code = "\n".join(ln for ln in src.splitlines() if not ln.lstrip().startswith("//"))
    keys = set(re.findall(r'\\"(\w+)\\":', code))
    assert keys == DASH_KEYS and len(DASH_KEYS) == 7
