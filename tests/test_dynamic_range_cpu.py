"""The oracle under exact scaling of a complex-float recording by 2^k (CPU).

x * 2^k is exact in float32, and every operation of the demodulator commutes exactly with it while no intermediate leaves the normal
range: inside the clean interval tests/rangeref.py predicts, the oracle's decisions, tone estimates, nin, timing and ppm must be the same
words, the soft magnitudes exactly 2^k times and the powers exactly 4^k times the k = 0 ones. One constant is not scaled with the signal:
the 1e-12 in the noise power (oracle fsk_demod_core: rx_nse_pow starts at 1E-12; the LLR stage: snse / Nsym + 1e-12f). rx_nse_pow,
SNRest and the soft bits are exact only where it is below half an ulp of what it meets (Regime.eps_clean); a frame without any noise
term keeps the bare constant at every k."""
import numpy as np
import pytest

import rangeref as rr
from parity import oracle_Sf


def _ldpc(oracle, M):
    import os
    code = oracle.parse_code_file(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pirip_amd", "data",
                                               "standin_256_512_4.code"))
    return oracle.OracleLdpc(code, M)


@pytest.mark.parametrize("name", list(rr.SHAPES))
def test_oracle_is_exactly_scale_invariant_over_the_clean_interval(oracle, name):
    sh = rr.SHAPES[name]
    x = rr.recording(oracle, sh, seed=3 + len(name))
    r0 = rr.demod(oracle, sh, x)
    reg = rr.Regime(x, sh, r0)
    lo, hi = reg.clean()
    assert r0["nframes"] >= 20 and np.count_nonzero(r0["stats"][:, 8]) >= 15
    # the interval is wide and holds the unnormalised s16 scale (k = 15); the 1e-12 range is a sub-interval of it at the bottom only
    assert lo <= -50 and hi >= 45, (lo, hi)
    eps = [k for k in range(lo, hi + 1) if reg.eps_clean(k)]
    assert eps == list(range(eps[0], hi + 1)) and eps[0] <= -5, (eps[0], hi)
    llr = _ldpc(oracle, sh["M"])
    l0 = llr.llr(r0["rx_filt"])
    silent = reg.first_nse == 0
    assert silent.any() and (~silent).any()                             # both kinds of frame are in the recording
    for k in range(lo, hi + 1):
        xk = rr.scaled(x, k)
        assert np.array_equal(np.ldexp(xk, -k), x), k                   # the input itself is exact
        rk = rr.demod(oracle, sh, xk)
        s = np.float32(2.0 ** k)
        assert (rk["nframes"], rk["consumed"]) == (r0["nframes"], r0["consumed"]), k
        assert np.array_equal(rk["bits"], r0["bits"]), k
        # f_est[0..3], norm_rx_timing, nin, ppm: the same words
        for col in (0, 1, 2, 3, 4, 6, 7):
            assert np.array_equal(rk["stats"][:, col].view(np.uint32), r0["stats"][:, col].view(np.uint32)), (k, col)
        assert np.array_equal(rk["rx_filt"], r0["rx_filt"] * s), k
        assert np.array_equal(rk["stats"][:, 8], r0["stats"][:, 8] * s * s), k                  # rx_sig_pow (starts at 0)
        if reg.eps_clean(k):
            assert np.array_equal(rk["stats"][~silent, 9], r0["stats"][~silent, 9] * s * s), k  # rx_nse_pow
            assert np.array_equal(rk["stats"][silent, 9], r0["stats"][silent, 9]), k            # 1e-12 / Nsym: not scaled
            assert np.array_equal(rk["stats"][:, 5].view(np.uint32), r0["stats"][:, 5].view(np.uint32)), k   # SNRest
            assert np.array_equal(llr.llr(rk["rx_filt"]), l0), k
    # below the 1e-12 range the constant shows: the noise power of a noisy frame is no longer 4^k times the k = 0 one
    k = lo
    rk = rr.demod(oracle, sh, rr.scaled(x, k))
    s = np.float32(2.0 ** k)
    assert not np.array_equal(rk["stats"][~silent, 9], r0["stats"][~silent, 9] * s * s)


@pytest.mark.parametrize("name", list(rr.SHAPES))
def test_ladder_brackets_every_boundary(oracle, name):
    """The predictor's ladder (used by the GPU tests): each pair of k straddles the boundary it claims, for the quantity it is computed
    from; where the oracle can show the crossing (the soft magnitudes, the frame power, |X|^2 through the estimator) it does."""
    sh = rr.SHAPES[name]
    x = rr.recording(oracle, sh, seed=3 + len(name))
    r0 = rr.demod(oracle, sh, x)
    reg = rr.Regime(x, sh, r0)
    L = reg.ladder()
    lo, hi = reg.clean()
    assert (L["clean_lo"], L["clean_hi"]) == (lo, hi) and lo < 0 < 15 < hi
    pairs = {"X2min": (reg.X2_min, -96), "tmin": (reg.tmax_min, -96), "min": (reg.quad_min(), -126), "max": (reg.quad_max(), 127)}
    for key, (v, e) in pairs.items():
        below, above = [L["%s_%s_2^%d" % (key, side, e)] for side in ("below", "above")]
        assert above == below + 1 and v * 4.0 ** below < 2.0 ** e <= v * 4.0 ** above, key
    # the soft magnitudes' squares cross 2^-96 where the predictor says (the oracle's own rx_filt at those k)
    t = [rr.demod(oracle, sh, rr.scaled(x, L["tmin_%s_2^-96" % side]))["rx_filt"].astype(np.float64) ** 2 for side in ("below", "above")]
    assert t[0][t[0] > 0].min() < 2.0 ** -96 <= t[1][t[1] > 0].min()
    # the top of the clean interval keeps every output finite; |X|^2's overflow k makes the estimator's Sf non-finite
    assert np.isfinite(rr.demod(oracle, sh, rr.scaled(x, hi))["stats"]).all()
    o = rr.oracle_fsk(oracle, sh)
    o.demod(rr.scaled(x, L["X2_overflow"]), oracle.IN_CF32)
    assert not np.isfinite(oracle_Sf(oracle, o, sh["Ndft"])).all()
    # the hand-over's sums-only overflow k: the frame power overflows, the soft magnitudes and the timing do not
    ko = rr.sums_overflow_k(oracle, x, sh, reg, x2_finite=False)
    assert ko is not None and ko > hi
    ro = rr.demod(oracle, sh, rr.scaled(x, ko))
    assert np.isinf(ro["stats"][:, 8]).any() and np.isfinite(ro["rx_filt"]).all() and np.isfinite(ro["stats"][:, 4]).all()
    assert not np.isinf(rr.demod(oracle, sh, rr.scaled(x, ko - 1))["stats"][:, 8]).any()

