"""Complex-float (cf32) inputs across their whole dynamic range on the device: a recording scaled by 2^k on the ladder
tests/rangeref.py predicts -- inside the clean interval, on either side of every range boundary of the kernels, and at overflow.

Scaling: inside the clean interval every kernel must be exactly scale invariant, like the oracle (tests/test_dynamic_range_cpu.py):
a range-dependent fast path or a constant hidden in a kernel is the only way to fail it. Parity: at every rung where no output
overflows, today's contract with the oracle; where the frame sums overflow, the same with inf / NaN counted equal where both hold them;
where |X|^2 overflows (the estimator's Sf holds inf), the point where kernel and oracle part ways is pinned exactly. Hand-over: the
fused FSK_LDPC soft bits equal the LLR stage's and the oracle's word for word."""
import numpy as np
import pytest

import rangeref as rr
from demodrun import same_words
from parity import RX_FILT_TOL, _compare

pytestmark = pytest.mark.gpu


def _hip(pirip_amd, sh, nstreams=1):
    lo, hi = rr.est_limits(sh)
    return pirip_amd.HipDemod(sh["Fs"], sh["Rs"], sh["M"], P=sh["P"], est_min=lo, est_max=hi, mask=sh["mask"],
                              in_format=pirip_amd.IN_CF32, nstreams=nstreams)


def _scaled_equal(rk, r0, k, reg):
    s = np.float32(2.0 ** k)
    assert (rk["nframes"], rk["consumed"]) == (r0["nframes"], r0["consumed"]), k
    assert np.array_equal(rk["bits"], r0["bits"]), k
    for col in (0, 1, 2, 3, 4, 6, 7):                                  # f_est, norm_rx_timing, nin, ppm
        same_words(rk["stats"][:, col], r0["stats"][:, col], (k, col))
    same_words(rk["rx_filt"], r0["rx_filt"] * s, k)
    same_words(rk["stats"][:, 8], r0["stats"][:, 8] * s * s, k)
    if reg.eps_clean(k):
        silent = reg.first_nse == 0                                    # frames without a noise term keep the bare 1e-12 / Nsym
        same_words(rk["stats"][:, 5], r0["stats"][:, 5], k)   # SNRest
        same_words(rk["stats"][~silent, 9], r0["stats"][~silent, 9] * s * s, k)
        same_words(rk["stats"][silent, 9], r0["stats"][silent, 9], k)


def _compare_nse_own(ro, rh, M):
    """_compare, with the noise power held to its own size: where the 1e-12 the oracle adds first and the kernels add last is not
    negligible (rungs below the 1e-12 range, silent frame edges), _compare's bar -- relative to the signal power -- is no bar for it."""
    no, nh = ro["stats"][:, 9].astype(np.float64), rh["stats"][:, 9].astype(np.float64)
    so = ro["stats"][:, 8].astype(np.float64)
    assert np.all(np.abs(nh - no) <= 2 * RX_FILT_TOL * np.maximum(np.maximum(so, no), 1e-45)), float(np.max(np.abs(nh - no) / np.maximum(no, 1e-45)))
    r2 = dict(rh, stats=rh["stats"].copy())
    r2["stats"][:, 9] = ro["stats"][:, 9]
    _compare(ro, r2, allow_near_tie_flips=True, M=M)


def _compare_nonfinite(ro, rh, M):
    """Where the frame sums overflow: the same stats words are inf / NaN on both sides (inf counted equal to inf, NaN to NaN), and
    everything else is held to _compare."""
    bad_o, bad_h = ~np.isfinite(ro["stats"]), ~np.isfinite(rh["stats"])
    assert np.array_equal(bad_o, bad_h), (np.argwhere(bad_o != bad_h)[:4])
    assert np.array_equal(ro["stats"][bad_o], rh["stats"][bad_h], equal_nan=True)
    assert np.isfinite(ro["rx_filt"]).all() and np.isfinite(rh["rx_filt"]).all()
    o2, r2 = dict(ro, stats=ro["stats"].copy()), dict(rh, stats=rh["stats"].copy())
    o2["stats"][bad_o] = 1.0
    r2["stats"][bad_h] = 1.0
    _compare_nse_own(o2, r2, M)


# Where |X|^2 overflows, the estimator's Sf holds inf and the kernels' arg-max / mask correlation and the oracle's serial search pick
# tones differently from some frame on (every soft magnitude stays finite). Pinned exactly, per case:
# (the kernel's consumed samples, the oracle's, the first frame whose bits, tone estimates or nin differ -- None: none; there every
# magnitude is zero, see below). Frame counts are equal.
X2_OVERFLOW_SPLIT = {
    "ts40_m2-auto": (46000, 46000, 4), "ts40_m4_mask-auto": (46000, 45970, 2), "ts20_m4_mask-auto": (23000, 23010, 2),
    "ts18_m2-auto": (21600, 21620, 7), "ts8_m2_mask-auto": (8802, 8802, 1), "ts40_m2-general": (46000, 46000, 3),
    "ts20_m4_mask-exact": (23010, 23010, 2), "ts10_m4-auto": (11500, 11500, None),
}


def _split_at(ro, rh):
    """The first frame at which bits, tone estimates or nin differ (None: none does)."""
    n = min(rh["nframes"], ro["nframes"])
    d = (rh["bits"][:n] != ro["bits"][:n]).any(axis=1) | (rh["stats"][:n, :4] != ro["stats"][:n, :4]).any(axis=1) \
        | (rh["stats"][:n, 6] != ro["stats"][:n, 6])
    f = np.flatnonzero(d)
    return int(f[0]) if f.size else None


CASES = [(n, "auto") for n in rr.SHAPES] + [("ts40_m2", "general"), ("ts20_m4_mask", "exact")]


@pytest.mark.parametrize("name,kernel", CASES, ids=["%s-%s" % c for c in CASES])
def test_scaled_recording_gives_scaled_words_and_keeps_parity(oracle, built_lib, monkeypatch, name, kernel):
    import pirip_amd
    if kernel == "general":
        monkeypatch.setenv("PIRIP_FORCE_GENERAL", "1")
    elif kernel == "exact":
        monkeypatch.setenv("PIRIP_KERNEL", "exact")
    sh = rr.SHAPES[name]
    x = rr.recording(oracle, sh, seed=3 + len(name))
    ro0 = rr.demod(oracle, sh, x)
    reg = rr.Regime(x, sh, ro0)
    ladder = reg.ladder()
    ko = rr.sums_overflow_k(oracle, x, sh, reg)
    if ko is not None:
        ladder["sums_overflow"] = ko
    h = _hip(pirip_amd, sh)
    assert h.kernel() == ("wave" if kernel == "auto" else kernel), h.kernel_name()
    rh0 = h.demod_host(x)
    seen = []
    for what, k in sorted(ladder.items(), key=lambda kv: kv[1]):
        h.reset()
        xk = rr.scaled(x, k)
        rh = h.demod_host(xk)
        ro = rr.demod(oracle, sh, xk)
        finite = np.isfinite(ro["rx_filt"]).all() and np.isfinite(ro["stats"]).all()
        seen.append((what, k, reg.is_clean(k), finite))
        if reg.is_clean(k):
            _scaled_equal(rh, rh0, k, reg)
        # parity with the oracle at every rung
        fin = finite and np.isfinite(rh["rx_filt"]).all() and np.isfinite(rh["stats"]).all()
        case = "%s-%s" % (name, kernel)
        if what == "X2_overflow" and case in X2_OVERFLOW_SPLIT:
            hc, oc, first = X2_OVERFLOW_SPLIT[case]
            assert rh["nframes"] == ro["nframes"] and (rh["consumed"], ro["consumed"]) == (hc, oc), (what, k, rh["consumed"], ro["consumed"])
            assert _split_at(ro, rh) == first, (what, k, _split_at(ro, rh))
            assert np.isfinite(ro["rx_filt"]).all() and np.isfinite(rh["rx_filt"]).all()
            if first is None:
                # no split, but every magnitude is zero: the oracle reports the bare 1e-12 / Nsym as noise power, the kernel 0, in the
                # same frames; every other word agrees
                assert not rh["rx_filt"].any()
                same_words(rh["rx_filt"], ro["rx_filt"], (what, k, "rx_filt"))
                same_words(rh["bits"], ro["bits"], (what, k, "bits"))
                d = rh["stats"][:, 9] != ro["stats"][:, 9]
                assert d.any() and (rh["stats"][d, 9] == 0).all() and (ro["stats"][d, 9] == np.float32(1e-12) / np.float32(50)).all()
                same_words(rh["stats"][:, :9], ro["stats"][:, :9], (what, k))
            continue
        assert (rh["nframes"], rh["consumed"]) == (ro["nframes"], ro["consumed"]), (what, k)
        if kernel == "exact":
            for f in ("bits", "rx_filt", "stats"):
                assert np.array_equal(rh[f], ro[f], equal_nan=f != "bits"), (what, k, f)
        elif not fin:
            _compare_nonfinite(ro, rh, sh["M"])
        elif reg.eps_clean(k):
            _compare(ro, rh, allow_near_tie_flips=True, M=sh["M"])
        else:
            _compare_nse_own(ro, rh, sh["M"])
    print(name, kernel, seen)
    # reset restores the k = 0 words after the overflow rungs
    h.reset()
    rh = h.demod_host(x)
    for f in ("bits", "rx_filt", "stats"):
        same_words(rh[f], rh0[f], f)


def test_codec2_shim_fsk_demod_is_scale_invariant(oracle, built_lib):
    """fsk_demod(fsk, bits, COMP *) (section C) on a cf32 wave shape: the bits and the nin sequence of x * 2^k are those of x."""
    import ctypes as C
    L = built_lib
    L.fsk_create_hbr.restype = C.c_void_p
    L.fsk_create_hbr.argtypes = [C.c_int] * 7
    L.fsk_set_freq_est_limits.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.fsk_nin.restype = C.c_uint32
    L.fsk_nin.argtypes = [C.c_void_p]
    L.fsk_demod.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.fsk_destroy.argtypes = [C.c_void_p]
    sh = rr.SHAPES["ts40_m2"]
    x = rr.recording(oracle, sh, seed=5)
    reg = rr.Regime(x, sh, rr.demod(oracle, sh, x))
    lo, hi = reg.clean()

    def run(xk):
        fsk = L.fsk_create_hbr(sh["Fs"], sh["Rs"], sh["M"], sh["P"], 50, -1, 100)
        L.fsk_set_freq_est_limits(fsk, *rr.est_limits(sh))
        pos, out, nins = 0, [], []
        while pos + L.fsk_nin(fsk) <= xk.shape[0]:
            nin = L.fsk_nin(fsk)
            bits = np.zeros(50, dtype=np.uint8)
            L.fsk_demod(fsk, bits.ctypes.data, np.ascontiguousarray(xk[pos:pos + nin]).ctypes.data)
            out.append(bits); nins.append(nin); pos += nin
        L.fsk_destroy(fsk)
        return np.stack(out), nins

    b0, n0 = run(x)
    ro = rr.demod(oracle, sh, x)
    assert np.array_equal(b0, ro["bits"])
    for k in (lo, -20, 15, hi):
        bk, nk = run(rr.scaled(x, k))
        assert np.array_equal(bk, b0) and nk == n0, k


LDPC_SHAPES = {     # the cf32 rows of test_ldpc.py's fused-chain test, plus 4-FSK at Ts 10
    "ts10_m2": dict(Fs=100000, Rs=10000, M=2, P=10, f1=10000, shift=10000, mask=0, Ndft=128),
    "ts20_m4_mask": rr.SHAPES["ts20_m4_mask"],
    "ts40_m2_p10": dict(Fs=40000, Rs=1000, M=2, P=10, f1=1000, shift=1000, mask=0, Ndft=512),
    "ts10_m4": rr.SHAPES["ts10_m4"],
}


@pytest.mark.parametrize("name", list(LDPC_SHAPES))
def test_fused_hand_over_soft_bits_equal_the_llr_stage_and_the_oracle(oracle, built_lib, name):
    """Binary16 soft bits word for word, three ways: the demodulator's fused hand-over (read back from the receiver's carried history),
    pirip_hip_ldpc_llr on the unfused rx_filt, the oracle's LLR mapping of the same rx_filt -- at k = 0 and 15, the top of the clean
    interval, below the quick path's 2^-96, where a symbol's sum - mx is denormal, and where the hand-over's frame sums overflow
    (fsk_demod_wave.hip: the quick path's upper bound; without it the corrected product turned +inf into NaN there). Where a call's sums
    overflow its soft bits are NaN before the store: all three write the erasure +0 for them, none hands a NaN on."""
    import torch
    import pirip_amd
    sh = LDPC_SHAPES[name]
    M = sh["M"]
    x = rr.recording(oracle, sh, seed=11 + M, frames=(12, 9), ebno_db=7.0)
    reg = rr.Regime(x, sh, rr.demod(oracle, sh, x))
    ks = {"k0": 0, "k15": 15, "clean_hi": reg.clean()[1], "tmin_below_2^-96": reg.ladder()["tmin_below_2^-96"],
          "oth_denormal": reg.k_oth_denormal()}
    ko = rr.sums_overflow_k(oracle, x, sh, reg, x2_finite=False)
    assert ko is not None
    ks["sums_overflow"] = ko
    code = oracle.parse_code_file(pirip_amd.STANDIN_CODE)
    nbits = 50 * (1 if M == 2 else 2)
    for what, k in ks.items():
        xk = rr.scaled(x, k)
        dem = _hip(pirip_amd, sh)
        filt = dem.demod_host(xk)["rx_filt"]
        nf = filt.shape[0]
        # the LLR stage on the unfused magnitudes, and the oracle's mapping
        d = torch.from_numpy(np.ascontiguousarray(filt)).cuda()
        L = pirip_amd.HipLdpc(pirip_amd.STANDIN_CODE, M)
        out = torch.zeros((nf, nbits), dtype=torch.float32, device="cuda")
        pirip_amd.binding._chk(L.L.pirip_hip_ldpc_llr(L.h, d.data_ptr(), nf, out.data_ptr(), 0), "llr")
        torch.cuda.synchronize()
        stage = out.cpu().numpy()
        want = oracle.OracleLdpc(code, M).llr(filt)
        # (a NaN soft bit -- overflowing sums make inf - inf -- is an erasure, +0, in all three: DESIGN.md 4.5)
        assert not np.isnan(stage).any() and not np.isnan(want).any(), (what, k)
        assert np.array_equal(stage, want), (what, k, np.argwhere(stage != want)[:4])
        # the fused chain, a few frames per call so that the carried history holds every soft bit of the call
        dem = _hip(pirip_amd, sh)
        F = pirip_amd.HipLdpc(pirip_amd.STANDIN_CODE, M)
        per_call = (2 * F.info.bits_per_frame) // nbits
        got, recs, pos = [], [], 0
        while len(got) < nf:
            host = np.ascontiguousarray(xk[pos:])[None]
            nsamp = host.shape[1]
            dd = torch.from_numpy(host).cuda()
            st = torch.zeros((1, per_call), dtype=torch.uint8, device="cuda")
            pl = torch.zeros((1, per_call, 32), dtype=torch.uint8, device="cuda")
            inf = torch.zeros((1, per_call, pirip_amd.LDPC_INFO_PER_CALL), dtype=torch.int32, device="cuda")
            nfr = torch.zeros(1, dtype=torch.int32, device="cuda")
            cons = torch.zeros(1, dtype=torch.int64, device="cuda")
            F.chain_batch(dem, dd.data_ptr(), nsamp * 8, nsamp, st.data_ptr(), pl.data_ptr(), inf.data_ptr(), nfr.data_ptr(), cons.data_ptr(), per_call)
            torch.cuda.synchronize()
            assert F.last_path_fused(), name
            n = int(nfr.cpu().numpy()[0])
            assert n > 0, (what, k, len(got))
            hist = F.llr_history(0).astype(np.float32)
            got += list(hist[len(hist) - n * nbits:].reshape(n, nbits))
            recs.append((st[0, :n].cpu().numpy(), pl[0, :n].cpu().numpy(), inf[0, :n].cpu().numpy()))
            pos += int(cons.cpu().numpy()[0])
        fused = np.stack(got)
        assert fused.shape == stage.shape, (what, k)
        assert not np.isnan(fused).any(), (what, k)
        assert np.array_equal(fused, stage), (what, k, np.argwhere(fused != stage)[:4])
        ws, wp, wi = oracle.OracleLdpc(code, M).rx(filt)
        assert np.array_equal(np.concatenate([r[0] for r in recs]), ws), (what, k)
        assert np.array_equal(np.concatenate([r[1] for r in recs]), wp), (what, k)
        assert np.array_equal(np.concatenate([r[2] for r in recs]), wi), (what, k)


@pytest.mark.parametrize("kernel", ["wave", "general"])
def test_streams_at_overflow_and_far_below_leave_their_neighbours_alone(oracle, built_lib, monkeypatch, kernel):
    """One batch of 8 streams: two at overflow k (the hand-over sums; |X|^2 as well), one at 2^-140 (every sample denormal or zero), the
    others at ordinary scales. Every other stream's words are those of its run alone."""
    import torch
    import pirip_amd
    if kernel == "general":
        monkeypatch.setenv("PIRIP_FORCE_GENERAL", "1")
    sh = rr.SHAPES["ts40_m2"]
    x = rr.recording(oracle, sh, seed=3 + len("ts40_m2"))
    reg = rr.Regime(x, sh, rr.demod(oracle, sh, x))
    ko = rr.sums_overflow_k(oracle, x, sh, reg)
    ko = ko if ko is not None else rr.sums_overflow_k(oracle, x, sh, reg, x2_finite=False)
    assert ko is not None
    ks = [0, ko, 15, reg.ladder()["X2_overflow"], -30, -140, 7, reg.clean()[1]]
    host = np.stack([rr.scaled(x, k) for k in ks])
    B, n = host.shape[0], host.shape[1]

    def run(h, arr):
        b = arr.shape[0]
        d = torch.from_numpy(np.ascontiguousarray(arr)).cuda()
        maxf = h.max_frames_for(n)
        bits = torch.zeros((b, maxf, h.Nbits), dtype=torch.uint8, device="cuda")
        filt = torch.zeros((b, maxf, sh["M"] * 50), dtype=torch.float32, device="cuda")
        st = torch.zeros((b, maxf, pirip_amd.STATS_PER_FRAME), dtype=torch.float32, device="cuda")
        nf = torch.zeros(b, dtype=torch.int32, device="cuda")
        cons = torch.zeros(b, dtype=torch.int64, device="cuda")
        h.demod_batch(d.data_ptr(), n * 8, n, bits.data_ptr(), maxf * h.Nbits, filt.data_ptr(), maxf * sh["M"] * 50,
                      st.data_ptr(), maxf * pirip_amd.STATS_PER_FRAME, nf.data_ptr(), cons.data_ptr(), maxf)
        torch.cuda.synchronize()
        return [x_.cpu().numpy() for x_ in (bits, filt, st, nf, cons)]

    hb = _hip(pirip_amd, sh, nstreams=B)
    assert hb.kernel() == kernel
    batch = run(hb, host)
    for s, k in enumerate(ks):
        if k in (ko, ks[3], -140):
            continue
        alone = run(_hip(pirip_amd, sh, nstreams=1), host[s:s + 1])
        for i, (a, b) in enumerate(zip(batch, alone)):
            same_words(a[s], b[0], (s, k, i))
