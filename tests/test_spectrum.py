"""include/pirip_hip.h section P on the device: the band monitor (pirip_hip_spec_*, pirip_amd.HipSpectrum, iq_spectrum).

Contract 1: rows and band entries equal the statement (tests/specref.py: numpy float32 around the oracle's kiss_fft) bit for bit.
Contract 2: any cutting of a stream into calls gives the one-shot output bit for bit, and a push writes exactly the rows nrows() announced.
Contract 3: a stream's output depends neither on the other streams, nor on the bands of the handle, nor on whether rows are stored."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import sigutil
import specref
import specshapes as sh

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "pirip_amd", "bin")
BAD_ARG, UNSUPPORTED = -1, -6
DASH_KEYS = set(json.load(open(os.path.join(ROOT, "tests", "golden", "dash_keys.json"))))


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_bands(a, b):
    return a.shape == b.shape and np.array_equal(_u32(a["power"]), _u32(b["power"])) and np.array_equal(_u32(a["peak"]), _u32(b["peak"])) and \
        np.array_equal(a["peak_bin"], b["peak_bin"])


def _dev(x):
    """the streams of specshapes.inputs as push() takes them: [nstreams, n, 2] uint8 or float32 on the device"""
    import torch
    if x.dtype == np.uint8:
        return torch.from_numpy(x.copy()).cuda()
    return torch.from_numpy(np.ascontiguousarray(x).view(np.float32).reshape(x.shape[0], x.shape[1], 2).copy()).cuda()


def _handle(nfft, hop, fmt, avg, nstreams=sh.NSTREAMS, bands=None):
    import pirip_amd
    return pirip_amd.HipSpectrum(sh.FS, nfft, hop=hop, avg=avg, nstreams=nstreams, bands=sh.bands(nfft) if bands is None else bands, in_format=sh.FMT[fmt])


def _run(h, xd, cuts, rows=None):
    """push xd in calls of the given lengths: (rows [nstreams, m, nfft] or None, band entries [nbands, m], rows per call)"""
    import torch
    import pirip_amd
    got_r, got_b, per_call, pos = [], [], [], 0
    for c in cuts:
        m = h.nrows(c)
        r, b = h.push(xd[:, pos:pos + c], rows=rows)
        assert b.shape[1] == m and (r is None or r.shape[1] == m)
        got_r.append(r); got_b.append(b); per_call.append(m)
        pos += c
    torch.cuda.synchronize()
    rws = None if rows is False else np.concatenate([r.cpu().numpy() for r in got_r], axis=1)
    bnd = np.concatenate([pirip_amd.HipSpectrum.band_rows(b) for b in got_b], axis=1)
    return rws, bnd, per_call


# ---- 1. exactness ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nfft,hop,fmt,avg", sh.CASES)
def test_rows_and_bands_equal_the_statement_bit_for_bit(built_lib, nfft, hop, fmt, avg):
    x = sh.inputs(nfft, hop, fmt, avg)
    want_r, want_b = sh.expected(nfft, hop, fmt, avg)
    h = _handle(nfft, hop, fmt, avg)
    assert np.array_equal(_u32(h.window()), _u32(specref.window(nfft)))
    assert h.scale == specref.scale(nfft, avg)
    for q, (_, lo, hi) in enumerate(sh.bands(nfft)):
        assert h.band_bins(q) == specref.band_bins(lo, hi, nfft, sh.FS), q
    rws, bnd, per_call = _run(h, _dev(x), sh.two_calls(x.shape[1]))
    assert sum(per_call) == 2
    assert rws.shape == want_r.shape and np.array_equal(_u32(rws), _u32(want_r))
    assert _same_bands(bnd, want_b)


# ---- 2. powers of two --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nfft,hop,fmt,avg", [c for c in sh.CASES if c[2] == "cf32"])
def test_powers_of_two_scale_exactly(built_lib, nfft, hop, fmt, avg):
    x = sh.inputs(nfft, hop, fmt, avg)
    want_r, want_b = sh.expected(nfft, hop, fmt, avg)
    for e in (20, -20):
        h = _handle(nfft, hop, fmt, avg)
        rws, bnd, _ = _run(h, _dev((x * np.float32(2.0 ** e)).astype(np.complex64)), sh.two_calls(x.shape[1]))
        k = np.float32(2.0 ** (2 * e))
        assert np.array_equal(_u32(rws), _u32(want_r * k))
        assert np.array_equal(_u32(bnd["power"]), _u32(want_b["power"] * k)) and np.array_equal(_u32(bnd["peak"]), _u32(want_b["peak"] * k))
        assert np.array_equal(bnd["peak_bin"], want_b["peak_bin"])


# ---- 3. cutting --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nfft,hop,fmt,avg", sh.CUT_CASES)
def test_any_cutting_equals_one_shot(built_lib, nfft, hop, fmt, avg):
    import torch
    import pirip_amd
    x = sh.inputs(nfft, hop, fmt, avg)
    n, nb, bs = x.shape[1], len(sh.bands(nfft)), sh.BS[fmt]
    xd = _dev(x)
    h = _handle(nfft, hop, fmt, avg)
    one_r, one_b, _ = _run(h, xd, [n])
    want_r, want_b = sh.expected(nfft, hop, fmt, avg)
    assert np.array_equal(_u32(one_r), _u32(want_r)) and _same_bands(one_b, want_b)
    R = 3                                                   # room for a row more than the input completes
    for cut in sh.cuttings(nfft, hop, avg, n):
        h.reset()
        rows = torch.full((sh.NSTREAMS, R, nfft), float("nan"), dtype=torch.float32, device="cuda")
        bands = torch.full((nb, R, 12), 0xEE, dtype=torch.uint8, device="cuda")
        canary_r, canary_b = rows.clone(), bands.clone()    # what a push that completes nothing is handed
        pos = done = 0
        for c in cut:
            m = h.nrows(c)
            out_r, out_b = (rows, bands) if m else (canary_r, canary_b)
            h.push_raw(xd.data_ptr() + pos * bs, n * bs, c, out_r.data_ptr() + done * nfft * 4, nfft, R * nfft, out_b.data_ptr() + done * 12, R)
            pos += c
            done += m
        torch.cuda.synchronize()
        assert done == 2
        r, b = rows.cpu().numpy(), pirip_amd.HipSpectrum.band_rows(bands)
        assert np.array_equal(_u32(r[:, :2]), _u32(one_r)) and _same_bands(b[:, :2], one_b)
        # the pushes that nrows() said complete nothing wrote nothing, and nobody wrote a third row
        assert torch.isnan(canary_r).all() and (canary_b == 0xEE).all() and np.isnan(r[:, 2]).all() and (bands[:, 2] == 0xEE).all()
    # reset, then the same input: the same rows
    h.reset()
    again_r, again_b, _ = _run(h, xd, [n])
    assert np.array_equal(_u32(again_r), _u32(one_r)) and _same_bands(again_b, one_b)


# ---- 4. independence ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nfft,hop,fmt,avg", [(256, 128, "cf32", 3), (1024, 512, "u8", 3), (4096, 4096, "cf32", 1), (4096, 2048, "u8", 3)])
def test_a_stream_depends_on_nothing_but_its_samples(built_lib, nfft, hop, fmt, avg):
    import torch
    import pirip_amd
    x = sh.inputs(nfft, hop, fmt, avg)
    n = x.shape[1]
    want_r, want_b = sh.expected(nfft, hop, fmt, avg)
    xd = _dev(x)
    all_bands = sh.bands(nfft)
    for r in range(sh.NSTREAMS):
        # the stream alone, with its own bands only
        mine = [q for q, b in enumerate(all_bands) if b[0] == r]
        h1 = _handle(nfft, hop, fmt, avg, nstreams=1, bands=[(0,) + all_bands[q][1:] for q in mine])
        rws, bnd, _ = _run(h1, xd[r:r + 1], sh.two_calls(n))
        assert np.array_equal(_u32(rws[0]), _u32(want_r[r])) and _same_bands(bnd, want_b[mine])
    # no rows stored: the band entries are the same bits
    h = _handle(nfft, hop, fmt, avg)
    rws, bnd, _ = _run(h, xd, sh.two_calls(n), rows=False)
    assert rws is None and _same_bands(bnd, want_b)
    # a handle with one band of the list, and one without bands
    for q in (sh.BAND["chan"][1], sh.BAND["wrap"], sh.BAND["all"]):
        hq = _handle(nfft, hop, fmt, avg, bands=[all_bands[q]])
        _, bnd, _ = _run(hq, xd, sh.two_calls(n), rows=False)
        assert _same_bands(bnd, want_b[q:q + 1]), q
    h0 = _handle(nfft, hop, fmt, avg, bands=[])
    rws, bnd, _ = _run(h0, xd, sh.two_calls(n))
    assert np.array_equal(_u32(rws), _u32(want_r)) and bnd.shape[0] == 0
    # padded strides: the padding stays as it was
    h.reset()
    rs, ss, bstr = nfft + 5, 2 * (nfft + 5) + 3, 4
    rows = torch.full((sh.NSTREAMS, ss), float("nan"), dtype=torch.float32, device="cuda")
    bands = torch.full((len(all_bands), bstr, 12), 0xEE, dtype=torch.uint8, device="cuda")
    h.push_raw(xd, n * sh.BS[fmt], n, rows, rs, ss, bands, bstr)
    torch.cuda.synchronize()
    r = rows.cpu().numpy()
    for j in range(2):
        assert np.array_equal(_u32(r[:, j * rs:j * rs + nfft]), _u32(want_r[:, j]))
        assert np.isnan(r[:, j * rs + nfft:(j + 1) * rs]).all()
    assert np.isnan(r[:, 2 * rs:]).all()
    assert _same_bands(pirip_amd.HipSpectrum.band_rows(bands)[:, :2], want_b) and (bands[:, 2:] == 0xEE).all()


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------------
def test_limits_and_bad_arguments(built_lib):
    import torch
    import pirip_amd
    L, Fs = built_lib, sh.FS
    Band = pirip_amd.SpecBand

    def create(Fs=Fs, fmt=1, nfft=256, hop=256, avg=1, nstreams=1, bands=(), nbands=None, bands_null=False, out_null=False):
        arr = (Band * max(len(bands), 1))(*[Band(*b) for b in bands])
        h = C.c_void_p()
        rc = L.pirip_hip_spec_create(Fs, fmt, nfft, hop, avg, nstreams, len(bands) if nbands is None else nbands,
                                     None if bands_null or not bands else C.addressof(arr), -1, None if out_null else C.byref(h))
        if rc == 0:
            assert L.pirip_hip_spec_destroy(h) == 0
        return rc

    assert create() == 0
    assert create(out_null=True) == BAD_ARG
    assert create(nstreams=0) == BAD_ARG and create(nbands=-1) == BAD_ARG and create(avg=0) == BAD_ARG
    assert create(nbands=1, bands_null=True) == BAD_ARG
    assert create(bands=[(1, 0, 0)]) == BAD_ARG and create(bands=[(-1, 0, 0)]) == BAD_ARG and create(bands=[(1, 0, 0)], nstreams=2) == 0
    assert create(bands=[(0, 5, 4)]) == BAD_ARG and create(bands=[(0, 4, 4)]) == 0
    assert create(bands=[(0, -Fs // 2 - 1, 0)]) == BAD_ARG and create(bands=[(0, -Fs // 2, 0)]) == 0
    assert create(bands=[(0, 0, Fs // 2)]) == BAD_ARG and create(bands=[(0, 0, Fs // 2 - 1)]) == 0
    assert create(Fs=Fs + 1, bands=[(0, -Fs // 2 - 1, Fs // 2 + 1)]) == BAD_ARG and create(Fs=Fs + 1, bands=[(0, -Fs // 2, Fs // 2)]) == 0   # an odd rate
    for fmt in (0, 2, 4, -1):
        assert create(fmt=fmt) == BAD_ARG
    assert create(fmt=3) == 0
    for nfft in (128, 512, 2048, 16384, 0):
        assert create(nfft=nfft, hop=nfft) == UNSUPPORTED, nfft
    for nfft in specref.NFFTS:
        assert create(nfft=nfft, hop=nfft // 4) == UNSUPPORTED and create(nfft=nfft, hop=2 * nfft) == UNSUPPORTED and create(nfft=nfft, hop=0) == UNSUPPORTED
        assert create(nfft=nfft, hop=nfft // 2) == 0 and create(nfft=nfft, hop=nfft) == 0
    assert create(avg=65537) == UNSUPPORTED and create(avg=65536) == 0
    assert create(Fs=(1 << 24) + 1) == UNSUPPORTED and create(Fs=1 << 24) == 0
    assert create(nstreams=65536) == UNSUPPORTED and create(nstreams=65535) == 0

    # push: the refusals between the two calls of a case change nothing
    nfft, hop, fmt, avg = 256, 128, "cf32", 3
    x = sh.inputs(nfft, hop, fmt, avg)
    want_r, want_b = sh.expected(nfft, hop, fmt, avg)
    n, nb = x.shape[1], len(sh.bands(nfft))
    xd = _dev(x)
    h = _handle(nfft, hop, fmt, avg)
    n1, n2 = sh.two_calls(n)
    assert h.nrows(n1) == 0 and h.nrows(n) == 2                 # (the first call completes no row here)
    rows = torch.full((sh.NSTREAMS, 2, nfft), float("nan"), dtype=torch.float32, device="cuda")
    bands = torch.zeros((nb, 2, 12), dtype=torch.uint8, device="cuda")
    good = dict(d_in=xd.data_ptr(), in_stride=n * 8, n=n1, d_rows=rows.data_ptr(), row_stride=nfft, stream_stride=2 * nfft, d_bands=bands.data_ptr(),
                band_stride=2)

    def push(hh=None, **kw):
        a = dict(good, **kw)
        return L.pirip_hip_spec_push(h.h if hh is None else hh, a["d_in"], a["in_stride"], a["n"], a["d_rows"], a["row_stride"], a["stream_stride"],
                                     a["d_bands"], a["band_stride"], 0)

    assert push() == 0
    good.update(d_in=xd.data_ptr() + n1 * 8, n=n2)               # the second call completes both rows
    assert push(hh=0) == BAD_ARG and push(d_in=None) == BAD_ARG and push(d_bands=None) == BAD_ARG
    assert push(n=0) == BAD_ARG and push(n=-1) == BAD_ARG
    assert push(d_in=good["d_in"] + 4) == BAD_ARG and push(in_stride=n * 8 + 4) == BAD_ARG and push(in_stride=n2 * 8 - 8) == BAD_ARG
    assert push(d_rows=good["d_rows"] + 2) == BAD_ARG and push(d_bands=good["d_bands"] + 2) == BAD_ARG
    assert push(row_stride=nfft - 1) == BAD_ARG and push(stream_stride=2 * nfft - 1) == BAD_ARG and push(band_stride=1) == BAD_ARG
    assert L.pirip_hip_spec_nrows(h.h, -1) == BAD_ARG and L.pirip_hip_spec_nrows(h.h, 1 << 53) == UNSUPPORTED
    assert L.pirip_hip_spec_band_bins(h.h, nb, None, None) == BAD_ARG and L.pirip_hip_spec_band_bins(h.h, -1, None, None) == BAD_ARG
    assert L.pirip_hip_spec_get_info(h.h, None) == BAD_ARG and L.pirip_hip_spec_reset(None, None) == BAD_ARG
    torch.cuda.synchronize()
    assert torch.isnan(rows).all()
    assert push() == 0
    torch.cuda.synchronize()
    assert np.array_equal(_u32(rows.cpu().numpy()), _u32(want_r)) and _same_bands(pirip_amd.HipSpectrum.band_rows(bands), want_b)
    # u8 samples are two bytes; a count of samples that would reach 2^53 (one stream: no stride to hold the rows apart)
    hu = _handle(256, 256, "u8", 1, nstreams=1, bands=[])
    xu = torch.zeros(1024, dtype=torch.uint8, device="cuda")
    pu = lambda d_in, n: L.pirip_hip_spec_push(hu.h, d_in, 0, n, None, 0, 0, None, 0, 0)
    assert pu(xu.data_ptr() + 1, 100) == BAD_ARG and pu(xu.data_ptr(), 1 << 53) == UNSUPPORTED and pu(xu.data_ptr(), 100) == 0
    assert pu(xu.data_ptr(), (1 << 53) - 100) == UNSUPPORTED and hu.nrows(412) == 2
    torch.cuda.synchronize()


# ---- 6. the point of it ------------------------------------------------------------------------------------------------------------------
def test_spectrum_finds_the_channels_the_channelizer_then_receives(built_lib, oracle):
    import torch
    import pirip_amd
    ob, cfg = oracle, sigutil.CFG3
    Fs, D, offsets, gains = 240000, 6, [-90000, -30000, 30001], [0.10, 0.08, 0.12]
    nbits = 1500
    bits = ob.get_test_bits(nbits)
    mx = pirip_amd.HipMux(Fs, D, offsets, gains=gains)
    Q = mx.Q
    nmod = nbits * (cfg["Fs"] // cfg["Rs"]) + 64
    n_in, n_wide = Q - 1 + nmod, nmod * D
    z = np.zeros((3, n_in, 2), dtype=np.float32)
    for c, lead in enumerate((0, 13, 29)):                      # three timing phases
        z[c, Q - 1 + lead:Q - 1 + lead + nbits * (cfg["Fs"] // cfg["Rs"])] = sigutil.mod_complex(ob, cfg, bits)
    zd = torch.from_numpy(z).cuda()
    wide = torch.zeros(n_wide * 2, dtype=torch.uint8, device="cuda")
    mx.batch(zd.data_ptr(), n_in * 8, n_in, wide.data_ptr(), n_wide * 2, m0=-(Q - 1))
    air = pirip_amd.HipAir(Fs, [(0, 0, 1.0, 0, 0)], 1, 1, sigma=0.02, seed=3)
    heard = torch.zeros(n_wide * 2, dtype=torch.uint8, device="cuda")
    air.push(wide, n_wide * 2, n_wide, heard, n_wide * 2)
    # the band monitor: a band around every candidate centre, the last two hold nothing
    bands = [(0, c - 15000, c + 15000) for c in offsets + [90000]] + [(0, -10000, 10000)]
    sp = pirip_amd.HipSpectrum(Fs, 1024, hop=512, avg=16, bands=bands)
    rows, b = sp.push(heard.view(1, n_wide, 2))
    torch.cuda.synchronize()
    br = sp.band_rows(b)
    assert rows.shape[1] == sp.nrows(0) + br.shape[1] and br.shape[1] >= 30
    occ = sp.occupied(br, noise_band=4, ratio_db=6.0)
    assert occ[:3].all() and not occ[3:].any()
    centres = [(lo + hi) // 2 for q, (_, lo, hi) in enumerate(bands) if occ[q].all()]
    assert centres == offsets
    ch = pirip_amd.HipChan(Fs, D, centres)
    no = ch.nout(n_wide)
    mod = torch.zeros((3, no * 8), dtype=torch.uint8, device="cuda")
    ch.batch(heard.data_ptr(), n_wide * 2, n_wide, mod.data_ptr(), no * 8)
    dem = pirip_amd.HipDemod(cfg["Fs"], cfg["Rs"], cfg["M"], P=cfg["P"], est_min=cfg["est_min"], est_max=cfg["est_max"], in_format=pirip_amd.IN_CF32, nstreams=3)
    R = dem.max_frames_for(no)
    dbits = torch.zeros((3, R, dem.Nbits), dtype=torch.uint8, device="cuda")
    nfr = torch.zeros(3, dtype=torch.int32, device="cuda")
    cons = torch.zeros(3, dtype=torch.int64, device="cuda")
    dem.demod_batch(mod.data_ptr(), no * 8, no, d_bits=dbits.data_ptr(), bits_stride=R * dem.Nbits, d_nframes=nfr.data_ptr(), d_consumed=cons.data_ptr(),
                    max_frames=R)
    torch.cuda.synchronize()
    nf, got, chans = nfr.cpu().numpy(), dbits.cpu().numpy(), mod.cpu().numpy().view(np.float32).reshape(3, no, 2)
    for c in range(3):
        o = ob.OracleFsk(cfg["Fs"], cfg["Rs"], cfg["M"], P=cfg["P"], est_min=cfg["est_min"], est_max=cfg["est_max"])
        ro = o.demod(chans[c], ob.IN_CF32, want_filt=False, want_stats=False)
        assert nf[c] == ro["nframes"] > 20 and np.array_equal(got[c, :nf[c]], ro["bits"]), c
        res = ob.put_test_bits(got[c, :nf[c]])
        assert res["bits"] >= 1000 and res["errors"] == 0, (c, res)


# ---- 7. the CLI --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nfft,hop,fmt,avg", [(1024, 512, "u8", 3), (4096, 4096, "cf32", 1)])
def test_cli_prints_the_bindings_figures(built_lib, tmp_path, nfft, hop, fmt, avg):
    x = sh.inputs(nfft, hop, fmt, avg)[2]                       # the stream of three FSK channels
    want_r, want_b = sh.expected(nfft, hop, fmt, avg)
    chan = [sh.bands(nfft)[q] for q in sh.BAND["chan"]]
    path = str(tmp_path / "capture.iq")
    x.tofile(path)
    cmd = [os.path.join(BIN, "iq_spectrum"), "--fs", str(sh.FS), "--format", fmt, "--nfft", str(nfft), "--avg", str(avg), "--block", "5000"] + \
          (["--half-overlap"] if hop < nfft else []) + [a for _, lo, hi in chan for a in ("--band", f"{lo}:{hi}")]
    p = subprocess.run(cmd + [path], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr
    lines = [ln.split() for ln in p.stdout.splitlines()]
    assert len(lines) == 2 * len(chan)
    scl = specref.scale(nfft, avg)
    for ln in lines:
        assert ln[0::2] == ["row", "band", "power_db", "peak_hz"]
        j, q = int(ln[1]), int(ln[3])
        e = want_b[sh.BAND["chan"][q]][j]
        nbins = specref.band_bins(chan[q][1], chan[q][2], nfft, sh.FS)[1]
        assert abs(float(ln[5]) - 10 * np.log10(float(e["power"]) * scl / nbins)) <= 1e-4
        assert abs(float(ln[7]) - specref.bin_hz(int(e["peak_bin"]), nfft, sh.FS)) <= 1e-3
    p = subprocess.run(cmd + ["--dash", path], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr
    out = [json.loads(ln) for ln in p.stdout.splitlines()]
    assert len(out) == 2
    for j, d in enumerate(out):
        assert set(d) == DASH_KEYS and len(d["SfdB"]) == nfft and d["Fs_Hz"] == sh.FS
        assert np.abs(np.array(d["SfdB"]) - specref.db(want_r[2][j], scl)).max() <= 1e-3
        assert d["fsk_lower_Hz"] == chan[0][1] and d["fsk_upper_Hz"] == chan[0][2] and d["SNRest_lin"] == 0 and d["norm_rx_timing"] == []
        assert len(d["f_est_Hz"]) == len(chan)
