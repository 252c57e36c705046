"""The life cycle of tests/test_binding_handles_cpu.py on the device: one handle of every class at the smallest size, closed twice; a
method of each closed handle raises PiripError in Python (the methods of that file's CASES), so the library never sees a NULL handle. The
handles that need others are built in dependency order and closed in reverse, then built again and only dropped, parents' names first:
each object's end then runs while the handles it borrowed are still referenced. Kernels run through construction only.

The composite handles take the arrangement of their own test modules: the transmit side and the channelized receiver of
tests/muxshapes.py's LOOP (tests/test_ping.py's _tx_side and tests/test_mux.py's _rx_handles), tests/test_ping.py's terminal and
repeater on them, and the receiver behind a decimator of tests/test_stream_rx.py."""
import gc

import pytest

import muxshapes as ms
from test_binding_handles_cpu import CASES

pytestmark = pytest.mark.gpu


def _closed_twice_and_dead(pirip_amd, h):
    method, args = CASES[type(h).__name__][2]
    assert h.h is not None
    h.close()
    h.close()
    assert h.h is None
    with pytest.raises(pirip_amd.PiripError, match="closed"):
        getattr(h, method)(*args)


def test_standalone_handles(built_lib):
    import pirip_amd
    for h in (pirip_amd.HipDemod(240000, 10000, 2, P=8, nstreams=1), pirip_amd.HipDecim(45), pirip_amd.HipLdpc(pirip_amd.STANDIN_CODE, 2),
              pirip_amd.HipTestBits(nstreams=1), pirip_amd.HipAir(240000, [(0, 0, 1.0, 0, 0)], 1, 1), pirip_amd.HipSpectrum(240000, 256)):
        _closed_twice_and_dead(pirip_amd, h)


def _composites(pirip_amd):
    """every handle that needs another, in dependency order: the name of each and the handle"""
    lp = ms.LOOP
    out = []

    def loop_side(tag):
        tx = pirip_amd.HipTx(ms.CODE, lp["mFs"], lp["Rs"], lp["M"], nstreams=4, f1=lp["f1"], shift=lp["shift"], gap=64)
        mux = pirip_amd.HipMux(lp["Fs"], lp["D"], lp["offsets"], gains=ms.LOOP_GAINS)
        block = 100 * lp["D"] * tx.Ts
        txs = pirip_amd.HipTxStream(tx, mux, block, 50 + lp["nframes"] * 544 + 64)
        dem = pirip_amd.HipDemod(lp["mFs"], lp["Rs"], lp["M"], P=lp["P"], est_min=lp["est_min"], est_max=lp["est_max"],
                                 in_format=pirip_amd.IN_CF32, nstreams=4)
        ld = pirip_amd.HipLdpc(ms.CODE, lp["M"], nstreams=4)
        ch = pirip_amd.HipChan(lp["Fs"], lp["D"], lp["offsets"])
        rx = pirip_amd.HipRx(dem, ldpc=ld, chan=ch, block=block)
        out.extend((tag + n, h) for n, h in (("tx", tx), ("mux", mux), ("txs", txs), ("dem", dem), ("ldpc", ld), ("chan", ch), ("rx", rx)))
        return tx, txs, rx

    tx, txs, rx = loop_side("repeater's ")
    out.append(("repeater", pirip_amd.HipRepeater(tx, txs, [1, 0, 3, 2], 2, filter=2, holdoff=1, max_burst=lp["nframes"],
                                                  pending=lp["nframes"] + 1, rx=rx)))
    tx, txs, rx = loop_side("terminal's ")
    out.append(("terminal", pirip_amd.HipPing(rx=rx, tx=tx, txs=txs, source=1, filter=1, frames=lp["nframes"], seq=True, period=1,
                                              first_call=[2, 3, 4, 5], max_bursts=1, log_entries=16)))
    dem40 = pirip_amd.HipDemod(40000, 1000, 2, P=10, est_min=500, est_max=15000, in_format=pirip_amd.IN_CF32, nstreams=8)
    dec6 = pirip_amd.HipDecim(6, out_s16=False)
    out += [("dem40", dem40), ("dec6", dec6), ("rx behind the decimator", pirip_amd.HipRx(dem40, dec=dec6, block=6 * 3000))]
    return out


def test_composite_handles_closed_in_reverse_then_only_dropped(built_lib):
    import torch
    import pirip_amd
    handles = _composites(pirip_amd)
    assert {type(h).__name__ for _, h in handles} == {"HipTx", "HipMux", "HipTxStream", "HipDemod", "HipLdpc", "HipChan", "HipRx", "HipDecim",
                                                      "HipRepeater", "HipPing"}
    for _, h in reversed(handles):
        _closed_twice_and_dead(pirip_amd, h)
    handles = _composites(pirip_amd)
    while handles:
        del handles[0]                      # the oldest name first: a handle others borrowed lives on in them until they have gone
    gc.collect()
    torch.cuda.synchronize()
