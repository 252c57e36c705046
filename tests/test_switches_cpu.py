"""The opt-in switches without a GPU (tests/switchshapes.py): every PIRIP_* name the library and its tools read has a decision in the
table; the decimator rows reach the kernel, tile and walk they claim by the launch rules restated in plain Python; and each arithmetic
row's input tells its arithmetics apart on the oracle alone, so a device that ignored the switch could not pass tests/test_switches.py."""
import glob
import os
import re

import numpy as np
import pytest

import sigutil
import switchshapes as ss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


# ---- the census ------------------------------------------------------------------------------------------------------------------------
def _switches_read_by_the_sources():
    names = set()
    for d in ("csrc", "tools"):
        for path in sorted(glob.glob(os.path.join(ROOT, "pirip_amd", d, "*"))):
            if os.path.isfile(path):
                names |= set(re.findall(r'getenv\("(PIRIP_[A-Za-z0-9_]+)"\)', _read(path)))
    return names


def test_every_switch_the_sources_read_has_a_decision():
    found = _switches_read_by_the_sources()
    assert len(found) > 30, "the scan found too little: did the sources move?"
    assert found == set(ss.SWITCHES), ("not in the table", sorted(found - set(ss.SWITCHES)), "no longer read", sorted(set(ss.SWITCHES) - found))


@pytest.mark.parametrize("name", sorted(ss.SWITCHES))
def test_a_switchs_decision_names_what_exists(name):
    kind, what = ss.SWITCHES[name]
    assert kind in ("test", "exempt")
    if kind != "test":
        assert len(what) > 20 and "\n" not in what
        return
    path, test = what.split("::")
    text = _read(path)
    assert re.search(r"^def %s\(" % re.escape(test), text, re.M), what
    assert re.search(name + r"\b", text), (name, "is not set anywhere in", path)


def test_the_wave_stop_switch_is_not_compiled():
    """the exemption's claim: the read sits inside #ifdef PIRIP_WAVE_TIMING and no build rule defines that macro"""
    src = _read("pirip_amd", "csrc", "fsk_demod_wave.hip")
    i = src.index('getenv("PIRIP_WAVE_STOP")')
    assert src.rfind("#ifdef PIRIP_WAVE_TIMING", 0, i) > src.rfind("#endif", 0, i)
    assert "PIRIP_WAVE_TIMING" not in _read("pirip_amd", "csrc", "Makefile")


# ---- the decimator's launch rules --------------------------------------------------------------------------------------------------------
def test_the_restated_rules_are_the_sources_rules():
    """the constants of the restatement, read from the source text: a changed rule fails here and sends the reader to switchshapes.py"""
    src = _read("pirip_amd", "csrc", "decim_kernels.hip")
    for needle in ("int tile = kThreads;", "+ 32 > 48 * 1024) tile /= 2;", "int tpw = 8;", "* nstreams < 8 * 256 * 6) tpw /= 2;",
                   "d->D == 45 || d->D == 50", "d->D == 6 || d->D == 9 || d->D == 10 || d->D == 18 || d->D == 30", "d->L == 79",
                   "d->shared && d->mode == kDecimExact && !(((uintptr_t)d_in | (uintptr_t)in_stride_bytes) & 1)",
                   "if (a.arith && !(g.head & 1))", "constexpr int kThreads = 256;"):
        assert needle in src, needle
    assert ss.FILL_WGS == 12288 and ss.filter_len(0.05) == 79 and ss.filter_len(0.0975) == 41


@pytest.mark.parametrize("D,tbw,kernel", ss.ARITH_ROWS)
def test_arithmetic_rows_reach_their_kernels(D, tbw, kernel):
    """mode 0 at an aligned address takes the row's kernel (which the opt-in modes must step aside from); modes 1 and 2 and any odd address
    take the general kernel, whose tap loop is the arithmetic one only at an even address; at least two tiles and a partial one"""
    plan = ss.decim_plan(D, tbw)
    n_in = ss.arith_n_in(D)
    l0 = ss.decim_launch(plan, n_in, ss.ARITH_STREAMS)
    assert l0["kernel"] == kernel and l0["tpw"] == 1
    for mode in (1, 2):
        lm = ss.decim_launch(plan, n_in, ss.ARITH_STREAMS, mode=mode)
        assert lm["kernel"] == "general" and lm["loop"] == "taps" and lm["tile"] == 256
        assert lm["ntiles"] >= 3 and lm["n_out"] % lm["tile"] != 0
        assert ss.decim_launch(plan, n_in, ss.ARITH_STREAMS, mode=mode, aligned=False)["loop"] == "table"
    assert l0["ntiles"] >= 3 and l0["n_out"] % l0["tile"] != 0


@pytest.mark.parametrize("D,tile", ss.LUT_ROWS)
def test_table_rows_take_the_general_kernels_table_loop(D, tile):
    plan = ss.decim_plan(D, lut=True)
    assert plan["shared"] == 0 and plan["tile"] == tile
    for aligned in (True, False):
        l = ss.decim_launch(plan, ss.arith_n_in(D), ss.ARITH_STREAMS, aligned=aligned)
        assert l["kernel"] == "general" and l["loop"] == "table" and l["ntiles"] >= 3 and l["n_out"] % tile != 0
    # without the switch the same shapes convert arithmetically
    assert ss.decim_launch(ss.decim_plan(D), ss.arith_n_in(D), ss.ARITH_STREAMS)["loop"] in ("taps", "n/a")


@pytest.mark.parametrize("r", ss.WALK_ROWS, ids=lambda r: r.name)
def test_walk_rows_reach_the_multi_tile_walk(r):
    plan = ss.decim_plan(r.D)
    n_in = ss.walk_n_in(r, plan)
    l = ss.decim_launch(plan, n_in, r.nstreams)
    assert (l["kernel"], l["tile"], l["ntiles"], l["tpw"]) == (r.kernel, r.tile, r.ntiles, r.tpw), l
    assert l["ntiles"] - (l["nwg"] - 1) * l["tpw"] == r.last                      # tiles the last workgroup of a stream walks
    assert l["n_out"] - (l["ntiles"] - 1) * l["tile"] == r.partial
    assert ss.decim_launch(plan, n_in, r.nstreams, env_tpw=1)["tpw"] == 1            # the call it is compared with
    assert r.pad % 2 == 0 and r.base % 2 == 0                                      # even addresses: the row's kernel, not the fallback
    assert r.base + r.nstreams * (2 * n_in + r.pad) + 64 + 2 * r.nstreams * l["n_out"] * 4 < 0.5e9, "bytes on the device"
    assert 0 in ss.walk_oracle_streams(r, plan) and r.nstreams - 1 in ss.walk_oracle_streams(r, plan)
    # what the rest of the suite runs -- a few streams of a few tiles -- never walks
    assert ss.decim_launch(plan, n_in, 5)["tpw"] == 1


def test_walk_rows_cover_all_three_kernels_and_the_long_walk():
    assert {r.kernel for r in ss.WALK_ROWS if r.tpw == 2} == {"general", "systolic", "shared"}
    assert any(r.tpw == 8 for r in ss.WALK_ROWS) and any(r.base for r in ss.WALK_ROWS)
    # for every kernel a row where a walk that began at tile blockIdx.x (not blockIdx.x * tpw) would leave the last tile to nobody
    nwg = lambda r: (r.ntiles + r.tpw - 1) // r.tpw
    assert {r.kernel for r in ss.WALK_ROWS if (nwg(r) - 1) + r.tpw < r.ntiles} == {"general", "systolic", "shared"}


# ---- the arithmetics can be told apart on the oracle alone ----------------------------------------------------------------------------------
@pytest.mark.parametrize("D,tbw,kernel", ss.ARITH_ROWS)
def test_decimator_arithmetics_differ_on_the_rows_bytes(oracle, D, tbw, kernel):
    """On the very bytes the device test runs (the three aligned streams of switchshapes.arith_host): mode 0 of the restatement is the
    scalar csdr loop; modes 1 and 2 differ from it and from each other in float words AND in s16 words, so neither output type of the
    device test can pass on a device that ignored a mode."""
    n_in = ss.arith_n_in(D)
    host = ss.arith_host(D)
    L = oracle.lib()
    tp, ntaps = oracle.decim_taps(D, tbw)
    assert ntaps == ss.filter_len(tbw) and len(tp) == ss.decim_plan(D, tbw)["Lp"]
    diff = {False: np.zeros(3, dtype=int), True: np.zeros(3, dtype=int)}
    for st in range(ss.ARITH_STREAMS):
        u8 = ss.arith_stream(host, D, "aligned", st)
        f = np.zeros(u8.shape, dtype=np.float32)
        L.oracle_convert_u8_f(u8.ctypes.data, f.ctypes.data, u8.size)
        y = np.zeros((n_in // D + 2, 2), dtype=np.float32)
        k = L.oracle_fir_decimate_cc(f.ctypes.data, y.ctypes.data, n_in, D, tp.ctypes.data, len(tp))
        out = {(m, s): oracle.decim_u8(u8, D, tbw, mode=m, out_s16=s) for m in (0, 1, 2) for s in (False, True)}
        assert k == out[(0, False)].shape[0] == ss.decim_launch(ss.decim_plan(D, tbw), n_in, 1)["n_out"]
        assert np.array_equal(out[(0, False)].view(np.uint32), y[:k].view(np.uint32))
        y0 = np.zeros_like(y)
        assert L.oracle_fir_decimate_cc_arith(0, u8.ctypes.data, y0.ctypes.data, n_in, D, tp.ctypes.data, len(tp)) == k
        assert np.array_equal(y0[:k].view(np.uint32), y[:k].view(np.uint32)), "mode 0 of the restatement is not the scalar csdr loop"
        assert L.oracle_fir_decimate_cc_arith(3, u8.ctypes.data, y0.ctypes.data, n_in, D, tp.ctypes.data, len(tp)) == -1
        for s in (False, True):
            diff[s] += [int((out[(a, s)] != out[(b, s)]).sum()) for a, b in ((0, 1), (0, 2), (1, 2))]
        # the variants stay what the header calls them: roundings of the same sum
        assert np.abs(out[(1, False)] - y[:k]).max() < 1e-6 and np.abs(out[(2, False)] - y[:k]).max() < 4e-6
    for s in (False, True):
        print(f"D = {D}, {'s16' if s else 'f32'}: words of {ss.ARITH_STREAMS} x {2 * k} that differ: exact/fma {diff[s][0]}, "
              f"exact/fma-raw {diff[s][1]}, fma/fma-raw {diff[s][2]}")
        assert diff[s].min() > 0, ("s16" if s else "f32", diff[s])


def test_fused_first_frame_shows_in_the_spectrum_after_one_frame(oracle):
    """after a whole run the spectrum has forgotten frame 0 (one-pole smoothing): what tells a fused frame 0 from an unfused one is Sf
    after that frame alone -- the device test of the prologue-off handle reads it there"""
    u8 = ss.fft_input(oracle, sigutil, "clean")[:1200]
    (r0, Sf0), (r1, Sf1) = ss.oracle_fft_run(oracle, sigutil, u8, False), ss.oracle_fft_run(oracle, sigutil, u8, True)
    assert r0["nframes"] == r1["nframes"] == 1
    assert (Sf0.view(np.uint32) != Sf1.view(np.uint32)).sum() > 0


@pytest.mark.parametrize("name", ss.FFT_INPUTS)
def test_fused_fft_multiply_moves_the_smoothed_spectrum(oracle, name):
    """the fused oracle's Sf differs from the unfused one's on each input (and with the switch flipped after frame 0, as the device's exact
    first-frame prologue has it); whether tone estimates, nin and bits still match is reported"""
    u8 = ss.fft_input(oracle, sigutil, name)
    r0, Sf0 = ss.oracle_fft_run(oracle, sigutil, u8, False)
    r1, Sf1 = ss.oracle_fft_run(oracle, sigutil, u8, True)
    r2, Sf2 = ss.oracle_fft_run(oracle, sigutil, u8, True, first_frame_unfused=True)
    assert oracle.lib().kiss_fft_oracle_get_fused_mul() == 0
    assert r0["nframes"] >= 100
    nd1, nd2 = int((Sf0.view(np.uint32) != Sf1.view(np.uint32)).sum()), int((Sf0.view(np.uint32) != Sf2.view(np.uint32)).sum())
    print(f"{name}: {r0['nframes']} frames; Sf words that differ from the unfused run: fused {nd1}, fused after frame 0 {nd2} of {Sf0.size}; "
          f"f_est equal {np.array_equal(r0['stats'][:, :4], r1['stats'][:, :4])}, nin equal {np.array_equal(r0['stats'][:, 6], r1['stats'][:, 6])}, "
          f"bits equal {np.array_equal(r0['bits'], r1['bits'])}")
    assert nd1 > 0 and nd2 > 0
    if name == "ppm400":
        assert (r0["stats"][:, 6] != 1200).any(), "the clock offset must move nin"
    # unfused, the replay in two calls is the one-call run: the flip is the only difference of the third run
    o = oracle.OracleFsk(240000, 10000, 2, P=24, est_min=500, est_max=25000)
    a = o.demod(u8[:1200], oracle.IN_CU8_FSKDEMOD)
    b = o.demod(u8[1200:], oracle.IN_CU8_FSKDEMOD)
    assert np.array_equal(np.concatenate([a["rx_filt"], b["rx_filt"]]).view(np.uint32), r0["rx_filt"].view(np.uint32))
