"""HipMac: include/pirip_hip.h section T on the binding's one handle base (pirip_amd/binding.py: _Handle, SIGNATURES, MacConfig, MacInfo).
It never computes on the CPU: every method is one C call."""
import ctypes as C

import numpy as np

from .binding import MacConfig, MacInfo, _dev, _Handle, _hip_stream


class HipMac(_Handle):
    """Half-duplex medium access (include/pirip_hip.h section T) attached to one HipPacket or HipPacketFec `pkt` that has a transmitter:
    while it lives, every call of pkt -- its own or a HipArq's -- senses carrier per receive channel, takes PIRIP_RX_BITS from the rows
    that the own transmitter produced, and lets the offer take bursts only after a slotted random backoff. rx_of_tx: per transmit channel
    the receive channel it listens on, None / -1 for an ungated channel; None for the whole argument: channel t listens on receive channel
    t. sense_mask: 1 a row with RX_SYNC is carrier, 2 a row whose SNRest >= sense_snr is, 3 both; slot_calls: calls per backoff slot; cw:
    an access draws 0 .. cw - 1 slots; ifs_calls: idle calls in front of the countdown; mute_calls: calls muted behind the own
    transmitter; txop_bursts: bursts per access; key: seeds the draws, the two ends of a link take different ones. pkt must outlive the
    HipMac and has one at most; close() detaches."""
    _c, _Info = "pirip_hip_mac", MacInfo

    TX_COUNTERS = ("accesses", "won", "backoff", "deferred", "bursts")
    RX_COUNTERS = ("carrier", "own", "muted")
    STATE = ("phase", "counter", "run", "quiet", "idle")

    def __init__(self, pkt, rx_of_tx=None, sense_mask=1, sense_snr=0.0, slot_calls=1, cw=8, ifs_calls=0, mute_calls=1, txop_bursts=1, key=1):
        self.pkt = pkt
        ntx = int(pkt.nchan)
        if rx_of_tx is None:
            rx_of_tx = range(ntx)
        rt = np.ascontiguousarray([-1 if c is None else int(c) for c in rx_of_tx], dtype=np.int32)
        if rt.size != ntx:
            raise ValueError("rx_of_tx: one value per transmit channel")
        cfg = MacConfig(int(sense_mask), float(sense_snr), int(slot_calls), int(cw), int(ifs_calls), int(mute_calls), int(txop_bursts),
                        int(key) & 0xFFFFFFFF)
        name = "pirip_hip_mac_create"
        self._create(name, pkt._ptr(name), C.byref(cfg), rt.ctypes.data)
        i = self.info
        self.ntx, self.nrx, self.rx_of_tx = i.ntx, i.nrx, rt.tolist()
        self._stats = None

    def set_stats(self, stats, stats_stride=None):
        """the stats rows (float32 [nrx, rows, STATS_PER_FRAME] tensor, or a raw device pointer with the stride in floats, or None) that
        go with the status rows of the push_records calls that follow"""
        if hasattr(stats, "stride") and stats_stride is None:
            stats_stride = int(stats.stride(0))
        self._stats = stats                                              # alive while the handle reads it
        self._call("pirip_hip_mac_set_stats", _dev(stats), int(stats_stride or 0))

    def stats(self):
        """(device pointer of the stats rows step 1 reads, floats per channel): set_stats' rows, or on a pkt with rx and sense bit 1 the
        receiver's rows of the last process / push; (0, 0) for none"""
        p, st = C.c_void_p(), C.c_size_t(0)
        self._call("pirip_hip_mac_stats", C.byref(p), C.byref(st))
        return int(p.value or 0), int(st.value)

    def counters(self):
        """dict of int64 arrays -- [ntx]: accesses, won, backoff, deferred, bursts; [nrx]: carrier, own, muted. Synchronises."""
        out = {k: np.zeros(self.ntx, dtype=np.int64) for k in self.TX_COUNTERS}
        out.update({k: np.zeros(self.nrx, dtype=np.int64) for k in self.RX_COUNTERS})
        self._call("pirip_hip_mac_get_counters", *(out[k].ctypes.data for k in self.TX_COUNTERS + self.RX_COUNTERS))
        return out

    def state(self, t):
        """checking aid: dict phase (MAC_IDLE / MAC_CONTEND / MAC_HOLD), counter, run, quiet, idle (-1 for an ungated channel).
        Synchronises."""
        v = [C.c_int(0) for _ in self.STATE]
        self._call("pirip_hip_mac_get_state", int(t), *(C.byref(x) for x in v))
        return {k: x.value for k, x in zip(self.STATE, v)}

    def reset(self, stream=None):
        """forgets the state and the counters (pkt.reset() does the same)"""
        self._call("pirip_hip_mac_reset", _hip_stream(stream))
