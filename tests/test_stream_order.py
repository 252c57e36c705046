"""include/pirip_hip.h's promise "enqueued on hip_stream; never synchronises", held on the device for every handle: each family of
tests/streamshapes.py runs its calls on a non-blocking side stream behind a spin kernel, with decoy inputs in place until the real ones
are copied in behind the gate (tests/streamgate.py), and must give the bytes of its synchronised run on the null stream -- twice, the
second time behind the family's reset; then two seeds on two gated streams at once. A step enqueued anywhere but on the caller's
stream runs during the gate and computes on the decoy; a call that waits for its stream returns after the gate has drained."""
import numpy as np
import pytest

import streamgate as sg
import streamshapes as ss

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _needs_sleep(built_lib):
    import torch
    if not hasattr(torch.cuda, "_sleep"):
        pytest.skip("torch.cuda._sleep is not available")


def test_rx_plain_gated(oracle, record_property):
    sg.run_family("rx_plain", oracle, record_property)


def test_rx_plain_pairs(oracle, record_property):
    sg.run_pair("rx_plain", oracle, record_property)


def test_rx_loop_gated(oracle, record_property):
    sg.run_family("rx_loop", oracle, record_property)


def test_rx_loop_pairs(oracle, record_property):
    sg.run_pair("rx_loop", oracle, record_property)


def test_chan_gated(record_property):
    sg.run_family("chan", None, record_property)


def test_chan_pairs(record_property):
    sg.run_pair("chan", None, record_property)


def test_decim_gated(record_property):
    sg.run_family("decim", None, record_property)


def test_decim_pairs(record_property):
    sg.run_pair("decim", None, record_property)


def test_mux_gated(record_property):
    sg.run_family("mux", None, record_property)


def test_mux_pairs(record_property):
    sg.run_pair("mux", None, record_property)


def test_tx_gated(record_property):
    sg.run_family("tx", None, record_property)


def test_tx_pairs(record_property):
    sg.run_pair("tx", None, record_property)


def test_txs_gated(record_property):
    sg.run_family("txs", None, record_property)


def test_txs_pairs(record_property):
    sg.run_pair("txs", None, record_property)


def test_tbits_gated(record_property):
    sg.run_family("tbits", None, record_property)


def test_tbits_pairs(record_property):
    sg.run_pair("tbits", None, record_property)


def test_spec_gated(record_property):
    sg.run_family("spec", None, record_property)


def test_spec_pairs(record_property):
    sg.run_pair("spec", None, record_property)


def test_air_gated(record_property):
    sg.run_family("air", None, record_property)


def test_air_pairs(record_property):
    sg.run_pair("air", None, record_property)


def test_rpt_gated(record_property):
    sg.run_family("rpt", None, record_property)


def test_rpt_pairs(record_property):
    sg.run_pair("rpt", None, record_property)


def test_ping_gated(record_property):
    sg.run_family("ping", None, record_property)


def test_ping_pairs(record_property):
    sg.run_pair("ping", None, record_property)


def test_div_gated(oracle, record_property):
    sg.run_family("div", oracle, record_property)


def test_div_pairs(oracle, record_property):
    sg.run_pair("div", oracle, record_property)


def test_pkt_gated(record_property):
    sg.run_family("pkt", None, record_property)


def test_pkt_pairs(record_property):
    sg.run_pair("pkt", None, record_property)


def test_fec_gated(record_property):
    sg.run_family("fec", None, record_property)


def test_fec_pairs(record_property):
    sg.run_pair("fec", None, record_property)


def test_arq_gated(record_property):
    sg.run_family("arq", None, record_property)


def test_arq_pairs(record_property):
    sg.run_pair("arq", None, record_property)


def test_arq_air_gated(record_property):
    sg.run_family("arq_air", None, record_property)


def test_arq_air_pairs(record_property):
    sg.run_pair("arq_air", None, record_property)


def test_ldpc_gated(oracle, record_property):
    sg.run_family("ldpc", oracle, record_property)


def test_ldpc_pairs(oracle, record_property):
    sg.run_pair("ldpc", oracle, record_property)


def test_mac_gated(record_property):
    sg.run_family("mac", None, record_property)


def test_mac_pairs(record_property):
    sg.run_pair("mac", None, record_property)


def test_gate_catches_a_step_on_another_stream(record_property):
    """The negative control: HipTx.frame on the gated side stream and HipTx.modulate on the null stream. modulate then runs during the
    gate, on the symbols that lay in the buffer before frame wrote it -- the decoy's --, so the IQ differs from the reference run's and
    equals what modulate alone makes of the decoy's symbols. Every byte read is initialised and in range."""
    import torch
    t = ss.TX
    want = sg.reference_of("tx", 0)
    # the decoy's symbols and counts: what frame makes of the decoy records (none: an all-zero status column starts no burst)
    dec = sg.build("tx", 0)
    dec.calls[0][1](0)
    dec.calls[1][1](0)
    torch.cuda.synchronize()
    decoy_syms, decoy_nsym = dec.outs["syms"].clone(), dec.outs["nsym"].clone()
    dec.reset(0)
    dec.outs["iq"].fill_(sg.CANARY)
    dec.calls[2][1](0)
    torch.cuda.synchronize()
    on_decoy = dec.outs["iq"].cpu().numpy().copy()
    dec.close()
    # repeat_records and frame on the side stream behind the gate, modulate on the null stream
    case = sg.build("tx", 0)
    gate_ms = ss.FAMILIES["tx"]["gate_ms"]
    g = sg.Gate(case, gate_ms)
    case.outs["syms"].copy_(decoy_syms)
    case.outs["nsym"].copy_(decoy_nsym)
    torch.cuda.synchronize()
    g.open()
    g.call(0)
    g.call(1)
    case.calls[2][1](0)                                    # the misrouted step
    g.check("modulate on the null stream")
    g.side.synchronize()
    torch.cuda.synchronize()
    record_property("enqueue_ms", round(g.enqueue_ms, 3))
    record_property("gate_ms", gate_ms)
    got = case.outs["iq"].cpu().numpy()
    ref = want["out:iq"].reshape(got.shape)
    assert np.array_equal(case.outs["syms"].cpu().numpy().reshape(-1), want["out:syms"]), "frame itself ran behind the gate, on the real records"
    assert not np.array_equal(got, ref), "a modulate enqueued on another stream than frame gave the reference run's bytes: the gate sees nothing"
    assert np.array_equal(got, on_decoy)
    assert not np.array_equal(on_decoy, ref)
    case.close()
    assert t["sigma"] > 0
