"""The comparison with the oracle every device test of the demodulators shares: tolerances, the frame-by-frame comparison
and the oracle's smoothed spectrum. The harness around it -- handles, runs in calls, the word-for-word comparison of two runs -- is
tests/demodrun.py."""
import numpy as np

RX_FILT_TOL = 1e-4        # relative to the peak magnitude of the compared block
SNR_TOL = 2e-3            # relative, SNRest (ratio of two reductions)
TIMING_TOL = 5e-5         # absolute, norm_rx_timing in symbols: the oracle's recursive timing phasor drifts ~1e-5 over 1224 steps


def _pair(ob, c, fmt_o, fmt_h, nstreams=1, mask=0, Nsym=50):
    import demodrun
    c = dict(c, Nsym=Nsym, mask=mask, fmt=fmt_h, band=False)
    return demodrun.make_oracle(ob, c), demodrun.make_handle(c, nstreams)


def _compare(ro, rh, tol=RX_FILT_TOL, allow_near_tie_flips=False, M=2):
    """Exact: frame count, consumed samples, tone estimates, nin sequence, bits.
    Tolerance: rx_filt, norm_rx_timing, SNRest. With allow_near_tie_flips (noisy inputs only) a
    differing bit is accepted -- and counted, the caller prints it -- only where the ORACLE's own
    decision margin (largest minus second largest tone magnitude of that symbol, any M) is below
    2*tol of the peak, i.e. where the two float32 evaluation orders straddle a tie; anything else is
    a failure. (tools/scale_check.py applies the same rule to 10^8 bits; tests/test_scale_check.py.)"""
    assert rh["nframes"] == ro["nframes"] and rh["consumed"] == ro["consumed"]
    assert np.array_equal(rh["stats"][:, :4], ro["stats"][:, :4]), "tone estimates differ"
    assert np.array_equal(rh["stats"][:, 6], ro["stats"][:, 6]), "nin sequence differs"
    nflips = 0
    if not np.array_equal(rh["bits"], ro["bits"]):
        diff = np.argwhere(rh["bits"] != ro["bits"])
        assert allow_near_tie_flips, f"{len(diff)} bit differences"
        filt = ro["rx_filt"]; peak = float(np.abs(filt).max())
        nbits = rh["bits"].shape[1]
        bps = 1 if M == 2 else 2
        nsym = nbits // bps
        assert filt.shape[1] == M * nsym
        for fr, b in diff:
            mags = np.sort(filt[fr].reshape(M, nsym)[:, b // bps])
            margin = float(mags[-1] - mags[-2]) / peak
            assert margin < 2 * tol, f"bit flip at frame {fr} bit {b} with margin {margin:.2e} of peak"
        nflips = len(diff)
    # The fine-timing estimate is the angle of a sum of (Nsym+1)*P terms; under noise that sum nearly cancels in a few frames per
    # 10^4 (tools/scale_check.py counts them: "ill-conditioned"), the two summation orders then give angles more than TIMING_TOL apart
    # and every interpolated magnitude of such a frame moves with the angle. Noisy tests accept a handful of those frames at a
    # looser magnitude tolerance; everywhere else -- and in every frame of a noise-free test -- both tolerances hold as stated.
    good = np.ones(ro["nframes"], dtype=bool)
    if ro["nframes"]:
        dt = np.abs(rh["stats"][:, 4] - ro["stats"][:, 4])                          # norm_rx_timing
        # (frames longer than 2400 samples: the caller scales tol by N / 2400, and the timing estimate -- the angle of a sum of the same
        #  correlator outputs -- moves with it: tools/fuzz_parity.py found 5.07e-5 on a noise-free Ts = 100, P = 4 stream, general kernel)
        ttol = TIMING_TOL * max(1.0, tol / RX_FILT_TOL)
        good = dt < ttol
        if allow_near_tie_flips:
            assert (~good).sum() <= max(2, ro["nframes"] // 300) and dt.max() < 100 * ttol, ((~good).sum(), dt.max())
            # ... and a frame is only excused when the ORACLE's own phasor sum is ill-conditioned: |t_c| / sum|terms| -- the
            # binding's "timing_cond", median 0.02-0.03 on these signals -- below 0.005, where a 1e-6 relative difference of the terms
            # moves the angle by more than TIMING_TOL / (2 pi 0.005) ~ 3e-5 symbols; a badly wrong frame with a healthy sum fails here
            if "timing_cond" in ro and (~good).any():
                assert np.all(ro["timing_cond"][~good] < 0.005 * max(1.0, tol / RX_FILT_TOL)), (ro["timing_cond"][~good], dt[~good])
        else:
            assert good.all(), dt.max()
    if ro["rx_filt"] is not None and rh["rx_filt"] is not None and ro["nframes"]:
        peak = max(float(np.max(np.abs(ro["rx_filt"]))), 1e-30)
        err = np.abs(rh["rx_filt"].astype(np.float64) - ro["rx_filt"].astype(np.float64)).max(axis=1) / peak
        # a frame's magnitudes are interpolated at its timing estimate: two estimates dt symbols apart (dt <= TIMING_TOL in a good frame) move
        # them by up to ~3 dt of the peak (the matched filter's slope), on top of the correlator tolerance -- found by tools/fuzz_parity.py:
        # one noisy frame in 1.6 x 10^4 noisy draws with dt = 4.0e-5 and an error of 1.013e-4
        assert np.all(err[good] < tol + 3.0 * dt[good]), float((err[good] - 3.0 * dt[good]).max())
        assert err[~good].max(initial=0.0) < 100 * tol, err[~good].max()
        sn_o, sn_h = ro["stats"][:, 5].astype(np.float64), rh["stats"][:, 5].astype(np.float64)
        rel = np.abs(sn_h - sn_o) / np.maximum(sn_o, 1e-9)
        inv = np.abs(1.0 / np.maximum(sn_h, 1e-9) - 1.0 / np.maximum(sn_o, 1e-9))
        # SNRest = sig/nse: on clean signals nse is ~1e-3 of sig, so compare the noise fraction
        assert np.all(((rel < SNR_TOL) | (inv < 5e-5))[good]), (rel.max(), inv.max())
        # rx_sig_pow / rx_nse_pow (what rtl_fsk -L logs as S and N): sums of Nsym terms in a different order
        so, sh = ro["stats"][:, 8].astype(np.float64), rh["stats"][:, 8].astype(np.float64)
        no, nh = ro["stats"][:, 9].astype(np.float64), rh["stats"][:, 9].astype(np.float64)
        assert np.all((np.abs(sh - so) <= 2 * tol * np.maximum(so, 1e-30))[good]) and np.all((np.abs(nh - no) <= 2 * tol * np.maximum(so, 1e-30))[good]), \
            (np.abs(sh / np.maximum(so, 1e-30) - 1).max(), (np.abs(nh - no) / np.maximum(so, 1e-30)).max())
    return nflips


def _oracle_field_Sf(oracle, o):
    """Address of ORACLE_FSK.Sf (the oracle's own getter: no test depends on the struct's layout)."""
    import ctypes as C
    o.l.oracle_fsk_get_Sf.restype = C.c_void_p
    o.l.oracle_fsk_get_Sf.argtypes = [C.c_void_p]
    return o.l.oracle_fsk_get_Sf(o.h)


def oracle_Sf(oracle, o, ndft=256):
    """the oracle's smoothed spectrum after its last frame"""
    import ctypes as C
    return np.ctypeslib.as_array(C.cast(_oracle_field_Sf(oracle, o), C.POINTER(C.c_float)), shape=(ndft,)).copy()
