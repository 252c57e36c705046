"""The harness every device test of the demodulators shares, between tests/sigutil.py (the signals) and tests/parity.py
(the comparison with the oracle): handle and oracle from one shape dict, pirip_hip_demod_batch in calls, the host read loop in ragged
chunks, the state readers, "equal word for word" and the one linear-interpolation body of the resamplers. Plain functions, no fixtures;
tests/test_demodrun_cpu.py holds the comparators to their strictness without a GPU.

A shape dict has Fs, Rs, M, P, est_min, est_max and optionally Nsym (50), mask (0: the peak estimator; else the comb's tone spacing),
fmt (the input format, pirip_amd.IN_* == oracle.IN_*; 0) and band (the band-only estimator; False)."""
import numpy as np

_WORD = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


def words(a):
    """the array as unsigned words of its item size"""
    a = np.ascontiguousarray(a)
    return a.view(_WORD[a.dtype.itemsize])


def same_words(a, b, what):
    """bit for bit: shape, dtype and every word (+0.0 is not -0.0, a NaN equals only its own payload)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    x, y = words(a), words(b)
    if not np.array_equal(x, y):
        bad = np.argwhere(x != y)
        raise AssertionError((what, "%d of %d words differ" % (len(bad), x.size), bad[:4].tolist(), a[tuple(bad[0])], b[tuple(bad[0])]))


def same_results(a, b, what, keys=None):
    """Two result dicts, or two lists of them per stream: the same keys on both sides, nframes and consumed equal, every array word for
    word. keys: compare these arrays only (the counts always)."""
    if isinstance(a, dict):
        a, b = [a], [b]
    assert len(a) == len(b), (what, len(a), len(b))
    for s, (x, y) in enumerate(zip(a, b)):
        assert set(x) == set(y), (what, s, "keys on one side only", sorted(set(x) ^ set(y)))
        for k in x:
            if isinstance(x[k], np.ndarray) or isinstance(y[k], np.ndarray):
                if keys is None or k in keys:
                    same_words(x[k], y[k], (what, s, k))
            elif keys is None or k in ("nframes", "consumed"):
                assert x[k] == y[k], (what, s, k, x[k], y[k])


def make_handle(c, nstreams=1, **kw):
    """HipDemod of a shape dict (kw overrides, e.g. est_min / est_max). Which kernel serves it is the caller's to assert."""
    import pirip_amd
    args = dict(P=c["P"], Nsym=c.get("Nsym", 50), est_min=c["est_min"], est_max=c["est_max"], mask=c.get("mask", 0), in_format=c.get("fmt", 0))
    h = pirip_amd.HipDemod(c["Fs"], c["Rs"], c["M"], nstreams=nstreams, **{**args, **kw})
    if c.get("band"):
        h.set_estimator_band_only(True)
    assert ("band-only" in h.kernel_name()) == bool(c.get("band")), h.kernel_name()
    return h


def make_oracle(oracle, c, est=None):
    """OracleFsk of a shape dict; est: another (est_min, est_max)"""
    lo, hi = est or (c["est_min"], c["est_max"])
    mask = c.get("mask", 0)
    return oracle.OracleFsk(c["Fs"], c["Rs"], c["M"], P=c["P"], Nsym=c.get("Nsym", 50), est_min=lo, est_max=hi,
                            tone_spacing=mask if mask else 100, mask=bool(mask))


def stream_state(h, s=0):
    """pirip_hip_get_stream_state: nin, norm_rx_timing, ppm, snr_est, SNRest, EbNodB, v_est, f_est[4], rx_sig_pow, rx_nse_pow as 13 words"""
    return np.frombuffer(h.stream_state(s), dtype=np.uint32)


def scalars(h, s=0):
    """pirip_hip_get_scalars: the eight stream scalars"""
    sc = np.zeros(8, dtype=np.float32)
    assert h.L.pirip_hip_get_scalars(h.h, s, sc.ctypes.data) == 0
    return sc


def run_calls(h, host, calls, before_call=None, watch=None, packed=False):
    """All B streams of host [B, L, ...] (any input format: the bytes per sample are the dtype's) through pirip_hip_demod_batch on handle
    h. calls[i] is the frame limit of call i, or (limit, frames every stream must make) where the input runs out first; every stream
    must make exactly that many. Between calls every stream's unconsumed samples are presented again from its own position.
    before_call(i, h) runs ahead of call i. packed: set_bit_packing(True) first, rows of packed bytes.
    Returns per stream nframes, consumed, bits, rx_filt, stats (views of the batch arrays) and, for the streams in watch (None: all), Sf,
    scalars and state (uint32 words)."""
    import torch
    import pirip_amd
    B, L = host.shape[0], host.shape[1]
    bps = host.dtype.itemsize * int(np.prod(host.shape[2:]))
    if packed:
        h.set_bit_packing(True)
    width = {"bits": (h.Nbits + 7) // 8 if packed else h.Nbits, "rx_filt": h.M * h.Nsym, "stats": pirip_amd.STATS_PER_FRAME}
    st = torch.cuda.current_stream().cuda_stream
    pos = np.zeros(B, dtype=np.int64)
    parts = {k: [] for k in width}
    for i, k in enumerate(calls):
        k, expect = k if isinstance(k, tuple) else (k, k)
        if before_call:
            before_call(i, h)
        n = int(L - pos.max())
        piece = host if not pos.any() else host[np.arange(B)[:, None], pos[:, None] + np.arange(n)[None, :]]
        dev = torch.from_numpy(np.ascontiguousarray(piece)).cuda()
        out = {key: torch.zeros((B, k, w), dtype=torch.uint8 if key == "bits" else torch.float32, device="cuda") for key, w in width.items()}
        nfr = torch.zeros(B, dtype=torch.int32, device="cuda"); cons = torch.zeros(B, dtype=torch.int64, device="cuda")
        h.demod_batch(dev.data_ptr(), n * bps, n, out["bits"].data_ptr(), k * width["bits"], out["rx_filt"].data_ptr(), k * width["rx_filt"],
                      out["stats"].data_ptr(), k * width["stats"], nfr.data_ptr(), cons.data_ptr(), k, st)
        torch.cuda.synchronize()
        assert (nfr.cpu().numpy() == expect).all(), ("call %d" % i, "frames wanted", expect, "made", nfr.cpu().numpy())
        for key in parts:
            assert not out[key][:, expect:].any(), ("call %d" % i, key, "rows past the frames made were written")
            parts[key].append(out[key][:, :expect].cpu().numpy())
        pos += cons.cpu().numpy()
    batch = {key: np.concatenate(v, axis=1) for key, v in parts.items()}
    F = batch["stats"].shape[1]
    res = [{"nframes": F, "consumed": int(pos[s]), **{key: batch[key][s] for key in batch}} for s in range(B)]
    for s in (range(B) if watch is None else watch):
        res[s].update(Sf=h.get_Sf(s), scalars=scalars(h, s), state=stream_state(h, s))
    return res


def host_chunks(h, buf, cuts):
    """The host read loop: the recording in demod_host calls cut at sample positions `cuts` (and at its end), the unconsumed tail carried
    in front of the next piece as a reader does. Returns the joined result."""
    parts, carry, last = [], buf[:0], 0
    for cut in list(cuts) + [buf.shape[0]]:
        piece = np.concatenate([carry, buf[last:cut]]); last = cut
        p = h.demod_host(piece)
        parts.append(p); carry = piece[p["consumed"]:]
    return {"nframes": sum(p["nframes"] for p in parts), "consumed": buf.shape[0] - carry.shape[0],
            **{k: np.concatenate([p[k] for p in parts]) for k, v in parts[0].items() if isinstance(v, np.ndarray)}}


def resample_at(x, t):
    """x [n, ...] read at positions t by linear interpolation with a float32 fraction (the right neighbour clamped to the last sample)"""
    i0 = np.floor(t).astype(int)
    fr = (t - i0).astype(np.float32).reshape((-1,) + (1,) * (x.ndim - 1))
    return ((1 - fr) * x[i0] + fr * x[np.minimum(i0 + 1, x.shape[0] - 1)]).astype(np.float32)
