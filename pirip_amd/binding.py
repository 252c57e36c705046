"""ctypes binding of libpirip_hip.so (include/pirip_hip.h, sections A, B, E, G, H, I, J, K, L, M, N, O, P, Q, R and S).

Device buffers are passed as raw device pointers (ints): with PyTorch, ``tensor.data_ptr()``
and ``torch.cuda.current_stream().cuda_stream``. Nothing here computes on the CPU; if the
library is missing or no HIP device is usable the calls raise PiripError.

Every prototype of the header has one entry in SIGNATURES, applied once by lib(); every handle class is a _Handle, which owns the
library, the C handle and its life cycle. tests/test_binding_abi_cpu.py holds the table and the structures below to the header.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# PIRIP_HIP_LIB: measurement builds only (e.g. the -DPIRIP_WAVE_TIMING library tools/phase_split.py reads its cycle split from)
_LIB = os.environ.get("PIRIP_HIP_LIB") or os.path.join(_HERE, "lib", "libpirip_hip.so")

IN_CU8_FSKDEMOD, IN_CU8_CSDR, IN_CS16, IN_CF32 = 0, 1, 2, 3
STATS_PER_FRAME = 10


class PiripError(RuntimeError):
    pass


class FskParams(C.Structure):
    _fields_ = [("Fs", C.c_int), ("Rs", C.c_int), ("M", C.c_int), ("P", C.c_int), ("Nsym", C.c_int),
                ("est_min", C.c_int), ("est_max", C.c_int), ("freq_est_type", C.c_int),
                ("tone_spacing", C.c_int), ("in_format", C.c_int)]


class FskInfo(C.Structure):
    _fields_ = [("Ts", C.c_int), ("N", C.c_int), ("Nmem", C.c_int), ("Ndft", C.c_int), ("Nbits", C.c_int),
                ("nin_max", C.c_int), ("nstreams", C.c_int), ("bytes_per_sample", C.c_int)]


class FskRecalled(C.Structure):
    """pirip_fsk_recalled: the constants held from recall of codec2, as data (include/pirip_hip.h)."""
    _fields_ = [("hann_denominator_ndft", C.c_int), ("tc", C.c_float), ("est_space_rs", C.c_float), ("nin_threshold", C.c_float),
                ("nin_step_div", C.c_int), ("s16_scale", C.c_float), ("u8d_offset", C.c_float), ("u8d_scale", C.c_float),
                ("ndft_rule", C.c_int), ("sf_power", C.c_int)]


class CaptureReport(C.Structure):
    _fields_ = [("segments", C.c_int32), ("segment_frames", C.c_int32), ("passes", C.c_int32), ("segments_rerun", C.c_int32),
                ("frames_demodulated", C.c_int64)]


class StreamState(C.Structure):
    """pirip_stream_state: what codec2 keeps in struct FSK between calls, 13 words (HipDemod.stream_state)"""
    _fields_ = [("nin", C.c_int)] + [(n, C.c_float) for n in ("norm_rx_timing", "ppm", "snr_est", "SNRest", "EbNodB", "v_est")] + \
               [("f_est", C.c_float * 4), ("rx_sig_pow", C.c_float), ("rx_nse_pow", C.c_float)]


class ChanInfo(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("Fs", "D", "ntaps", "ntaps_padded", "ninputs", "nchan", "out_s16", "device")]


class MuxInfo(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("Fs", "D", "kind", "ntaps", "ntaps_padded", "Q", "noutputs", "nchan", "out_format", "device")]


class TxInfo(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("Fs", "Rs", "M", "Ts", "n", "k", "bits_per_frame", "data_bytes", "preamble_syms", "frame_syms",
                                       "nstreams", "device")]


class TxsInfo(C.Structure):
    _fields_ = [("block", C.c_int64), ("queue_syms", C.c_int64)] + \
               [(n, C.c_int) for n in ("S", "H", "nchan", "noutputs", "out_format", "device")]


class RptInfo(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("nrx", "nchan", "source_byte", "filter_byte", "holdoff_calls", "max_burst_frames", "pending_records",
                                       "has_rx", "rx_rows", "device")]


class PingConfig(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("nrx", "source_byte", "filter_byte", "frames_per_burst", "seq", "period_calls")] + \
               [("first_call", C.POINTER(C.c_int32)), ("max_bursts", C.c_int64), ("log_entries", C.c_int), ("nin0", C.c_int)]


class PingEntry(C.Structure):
    _fields_ = [("t_samples", C.c_int64), ("call", C.c_int32), ("row", C.c_int32), ("S", C.c_float), ("N", C.c_float), ("SNRest", C.c_float),
                ("ecdd", C.c_int32), ("eraw", C.c_int32), ("source", C.c_uint8), ("seq", C.c_uint8), ("status", C.c_uint8), ("iters", C.c_uint8)]


# pirip_ping_entry as a numpy structured dtype (40 bytes, the C layout): what HipPing.log returns
PING_ENTRY_DTYPE = [("t_samples", "<i8"), ("call", "<i4"), ("row", "<i4"), ("S", "<f4"), ("N", "<f4"), ("SNRest", "<f4"), ("ecdd", "<i4"),
                    ("eraw", "<i4"), ("source", "u1"), ("seq", "u1"), ("status", "u1"), ("iters", "u1")]


class PingInfo(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("nrx", "nchan", "source_byte", "filter_byte", "frames_per_burst", "seq", "period_calls", "log_entries",
                                       "nin0", "has_rx", "rx_rows", "data_bytes", "device")] + [("max_bursts", C.c_int64)]


class AirPath(C.Structure):
    """pirip_air_path: received stream, transmitted stream, delay in samples, carrier offset in Hz, real gain"""
    _fields_ = [("rx", C.c_int32), ("tx", C.c_int32), ("delay", C.c_int32), ("offset_hz", C.c_int32), ("gain", C.c_float)]


class AirPathEx(C.Structure):
    """pirip_air_path_ex: AirPath and the path's clock offset in parts per billion"""
    _fields_ = AirPath._fields_ + [("clock_ppb", C.c_int32)]


class AirFade(C.Structure):
    """pirip_air_fade: index of the path the fade is attached to, Doppler spread in millihertz, Rician K (0: Rayleigh), key of its draws"""
    _fields_ = [("path", C.c_int32), ("doppler_millihz", C.c_int32), ("rice_k", C.c_float), ("key", C.c_uint32)]


class AirInfo(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("Fs", "ntx", "nrx", "npaths", "in_format", "out_format", "max_delay", "device")]


class SpecBand(C.Structure):
    """pirip_spec_band: the stream, and the band's edges in Hz, -Fs/2 <= lo <= hi < Fs/2"""
    _fields_ = [("stream", C.c_int32), ("lo_hz", C.c_int32), ("hi_hz", C.c_int32)]


class SpecInfo(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("Fs", "in_format", "nfft", "hop", "avg", "nstreams", "nbands", "device")] + [("scale", C.c_double)]


class DivConfig(C.Structure):
    """pirip_div_config: branches per group, samples per symbol, the first call's samples, skew in samples, rows per call, ring entries"""
    _fields_ = [(n, C.c_int) for n in ("branches", "samples_per_symbol", "nin0", "max_skew_samples", "max_rows", "log_entries")]


class DivEntry(C.Structure):
    _fields_ = [("t_samples", C.c_int64), ("iters", C.c_int32), ("pcc", C.c_int32), ("eraw", C.c_int32), ("members", C.c_uint8),
                ("solo_ok", C.c_uint8), ("status", C.c_uint8), ("pad", C.c_uint8)]


# pirip_div_entry as a numpy structured dtype (24 bytes, the C layout): what HipDiversity.log and .last return
DIV_ENTRY_DTYPE = [("t_samples", "<i8"), ("iters", "<i4"), ("pcc", "<i4"), ("eraw", "<i4"), ("members", "u1"), ("solo_ok", "u1"),
                   ("status", "u1"), ("pad", "u1")]


class DivInfo(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("groups", "branches", "samples_per_symbol", "nin0", "max_skew_samples", "max_rows", "log_entries",
                                       "pending", "slots", "n", "data_bytes", "device")]


class PktConfig(C.Structure):
    """pirip_pkt_config: receive channels, src of frames sent, filtered byte 0 or -1, accepted dst or -1, fragments per packet, records of
    a pending ring, packets of a receive ring"""
    _fields_ = [(n, C.c_int) for n in ("nrx", "source_byte", "filter_byte", "address", "max_frags", "pending_records", "ring_entries")]


class PktEntry(C.Structure):
    _fields_ = [("seq", C.c_int64), ("call", C.c_int32), ("row", C.c_int32), ("length", C.c_int32), ("src", C.c_uint8), ("dst", C.c_uint8),
                ("id", C.c_uint8), ("nfrag", C.c_uint8)]


# pirip_pkt_entry as a numpy structured dtype (24 bytes, the C layout): what HipPacket.packets returns
PKT_ENTRY_DTYPE = [("seq", "<i8"), ("call", "<i4"), ("row", "<i4"), ("length", "<i4"), ("src", "u1"), ("dst", "u1"), ("id", "u1"), ("nfrag", "u1")]


class PktInfo(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("nrx", "nchan", "source_byte", "filter_byte", "address", "max_frags", "pending_records", "ring_entries",
                                       "cap", "max_packet", "has_rx", "rx_rows", "data_bytes", "device")]


class PktFecConfig(C.Structure):
    """pirip_pkt_fec_config: parity fragments of a packet at most (1 .. 16), parity fragments per 100 data fragments (1 .. 100)"""
    _fields_ = [(n, C.c_int) for n in ("max_parity", "parity_pct")]


class PktFecInfo(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("enabled", "max_parity", "parity_pct", "max_burst_frames")]


class ArqConfig(C.Structure):
    """pirip_arq_config: segments in flight, calls until a segment is sent again, transmissions before the session is broken, segments of
    a submit queue, segments of an output ring"""
    _fields_ = [(n, C.c_int) for n in ("window", "rto_calls", "max_tries", "queue_entries", "out_entries")]


class ArqEntry(C.Structure):
    _fields_ = [("seq", C.c_int64), ("call", C.c_int32), ("length", C.c_int32)]


# pirip_arq_entry as a numpy structured dtype (16 bytes, the C layout): what HipArq.delivered returns
ARQ_ENTRY_DTYPE = [("seq", "<i8"), ("call", "<i4"), ("length", "<i4")]


class ArqInfo(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("nchan", "window", "rto_calls", "max_tries", "queue_entries", "out_entries", "max_payload", "acklen",
                                       "device")]


class MacConfig(C.Structure):
    """pirip_mac_config: what counts as carrier and from which SNRest on, calls per backoff slot, slots to draw from, idle calls in front
    of the countdown, calls muted behind the own transmitter, bursts per access, the key of the draws"""
    _fields_ = [("sense_mask", C.c_int), ("sense_snr", C.c_float)] + \
               [(n, C.c_int) for n in ("slot_calls", "cw", "ifs_calls", "mute_calls", "txop_bursts")] + [("key", C.c_uint32)]


class MacInfo(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("ntx", "nrx", "sense_mask")] + [("sense_snr", C.c_float)] + \
               [(n, C.c_int) for n in ("slot_calls", "cw", "ifs_calls", "mute_calls", "txop_bursts")] + [("key", C.c_uint32), ("device", C.c_int)]


MAC_IDLE, MAC_CONTEND, MAC_HOLD = 0, 1, 2


# pirip_spec_band_row as a numpy structured dtype (12 bytes, the C layout): what HipSpectrum.push's band entries are on the host
SPEC_BAND_ROW_DTYPE = [("power", "<f4"), ("peak", "<f4"), ("peak_bin", "<i4")]


class LdpcInfo(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("n", "k", "bits_per_frame", "data_bytes", "nbits_per_call", "max_iter", "nstreams")] + \
               [("name", C.c_char * 64)]


class ChainGroup(C.Structure):
    """struct pirip_chain_group (include/pirip_hip.h)"""
    _fields_ = [("dem", C.c_void_p), ("ldpc", C.c_void_p), ("d_in", C.c_void_p), ("d_status", C.c_void_p), ("d_payload", C.c_void_p),
                ("d_info", C.c_void_p), ("d_stats", C.c_void_p), ("d_nframes", C.c_void_p), ("d_consumed", C.c_void_p)]


RX_TRIAL_SYNC, RX_SYNC, RX_BITS, RX_BIT_ERRORS = 1, 2, 4, 8
LDPC_INFO_PER_CALL = 10
STANDIN_CODE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "standin_256_512_4.code")


def _signatures():
    vp, i32, i64, u64, sz, f32, cs, P = C.c_void_p, C.c_int, C.c_int64, C.c_uint64, C.c_size_t, C.c_float, C.c_char_p, C.POINTER
    return {
        # section A: batch-of-streams demodulator
        "pirip_hip_create": (i32, [P(FskParams), i32, i32, P(vp)]),
        "pirip_hip_recalled_defaults": (None, [P(FskRecalled)]),
        "pirip_hip_create_recalled": (i32, [P(FskParams), P(FskRecalled), i32, i32, P(vp)]),
        "pirip_hip_destroy": (i32, [vp]),
        "pirip_hip_get_info": (i32, [vp, P(FskInfo)]),
        "pirip_hip_get_kernel": (i32, [vp]),
        "pirip_hip_set_exact_first_frame": (i32, [vp, i32]),
        "pirip_hip_get_kernel_name": (i32, [vp, cs, sz]),
        "pirip_hip_reset": (i32, [vp, vp]),
        "pirip_hip_clear_estimators": (i32, [vp, vp]),
        "pirip_hip_demod_batch": (i32, [vp, vp, sz, i64, vp, sz, vp, sz, vp, sz, vp, vp, i64, vp]),
        "pirip_hip_demod_capture": (i32, [vp, vp, i64, vp, vp, vp, i64, P(i64), P(i64), P(CaptureReport), vp]),
        "pirip_hip_demod_capture_host": (i32, [vp, vp, i64, vp, vp, vp, i64, P(i64), P(i64), P(CaptureReport)]),
        "pirip_hip_demod_host": (i32, [vp, vp, i64, vp, vp, vp, i64, P(i64), P(i64)]),
        "pirip_hip_nin0": (i32, [vp]),
        "pirip_hip_set_bit_packing": (i32, [vp, i32]),
        "pirip_hip_set_estimator_band_only": (i32, [vp, i32]),
        "pirip_hip_set_launch_tail_first": (i32, [vp, i32]),
        "pirip_hip_get_launch_resident_blocks": (i32, [vp]),
        "pirip_hip_launch_first_tail_block": (i32, [i32, i32, i32, i32]),
        "pirip_hip_set_burst_mode": (i32, [vp, i32]),
        "pirip_hip_get_Sf": (i32, [vp, i32, vp]),
        "pirip_hip_enable_eye": (i32, [vp, i32]),
        "pirip_hip_get_eye": (i32, [vp, i32, i32, vp, vp, vp]),
        "pirip_hip_get_scalars": (i32, [vp, i32, vp]),
        "pirip_hip_get_stream_state": (i32, [vp, i32, P(StreamState)]),
        "pirip_hip_set_freq_est_limits": (i32, [vp, i32, i32]),
        # section B: csdr front end, and B2: synthetic Tx
        "pirip_hip_decim_create": (i32, [i32, f32, i32, i32, P(vp)]),
        "pirip_hip_decim_destroy": (i32, [vp]),
        "pirip_hip_decim_taps": (i32, [vp, vp, P(i32)]),
        "pirip_hip_decim_set_arith": (i32, [vp, i32]),
        "pirip_hip_decim_get_arith": (i32, [vp]),
        "pirip_hip_decim_nout": (i64, [vp, i64]),
        "pirip_hip_decim_batch": (i32, [vp, vp, sz, i64, vp, sz, i32, vp]),
        "pirip_hip_synth_cu8": (i32, [i32, i32, i32, i32, vp, i32, vp, vp, sz, i64, vp, sz, i64, f32, f32, u64, vp]),
        # section E: FSK_LDPC receive
        "pirip_hip_ldpc_create": (i32, [cs, i32, i32, i32, i32, P(vp)]),
        "pirip_hip_ldpc_destroy": (i32, [vp]),
        "pirip_hip_ldpc_get_info": (i32, [vp, P(LdpcInfo)]),
        "pirip_hip_ldpc_reset": (i32, [vp, vp]),
        "pirip_hip_ldpc_get_llr_history": (i32, [vp, i32, vp]),
        "pirip_hip_ldpc_get_layout_conflicts": (i32, [vp, P(i32), P(i32)]),
        "pirip_hip_ldpc_rx_batch": (i32, [vp, vp, sz, vp, i32, vp, vp, vp, vp]),
        "pirip_hip_fsk_ldpc_rx_batch": (i32, [vp, vp, vp, sz, i64, vp, vp, vp, vp, sz, vp, vp, i64, vp]),
        "pirip_hip_fsk_ldpc_last_path": (i32, [vp]),
        "pirip_hip_fsk_ldpc_rx_batch_groups": (i32, [P(ChainGroup), i32, sz, i64, sz, i64, vp]),
        "pirip_hip_ldpc_rx_host": (i32, [vp, vp, i32, vp, vp, vp]),
        "pirip_hip_ldpc_llr": (i32, [vp, vp, i32, vp, vp]),
        "pirip_hip_ldpc_decode_llr": (i32, [vp, vp, i32, vp, vp, vp]),
        # section G: streaming receiver
        "pirip_hip_rx_create": (i32, [vp, vp, vp, i64, P(vp)]),
        "pirip_hip_rx_destroy": (i32, [vp]),
        "pirip_hip_rx_max_frames": (i64, [vp]),
        "pirip_hip_rx_input": (i32, [vp, P(vp), P(sz)]),
        "pirip_hip_rx_process": (i32, [vp, vp, sz, vp, sz, vp, vp, vp, vp, sz, vp, vp]),
        "pirip_hip_rx_push": (i32, [vp, vp, sz, vp, sz, vp, sz, vp, vp, vp, vp, sz, vp, vp]),
        "pirip_hip_rx_get_counters": (i32, [vp, vp, vp]),
        "pirip_hip_rx_reset": (i32, [vp, vp]),
        # section H: channelizer
        "pirip_hip_chan_create": (i32, [i32, i32, f32, i32, i32, i32, vp, vp, i32, P(vp)]),
        "pirip_hip_chan_destroy": (i32, [vp]),
        "pirip_hip_chan_get_info": (i32, [vp, P(ChanInfo)]),
        "pirip_hip_chan_taps": (i32, [vp, vp, P(i32)]),
        "pirip_hip_chan_nout": (i64, [vp, i64]),
        "pirip_hip_chan_batch": (i32, [vp, vp, sz, i64, i64, vp, sz, vp]),
        "pirip_hip_rx_create_chan": (i32, [vp, vp, vp, i64, P(vp)]),
        # section I: FSK_LDPC transmit
        "pirip_hip_tx_create": (i32, [cs, i32, i32, i32, i32, i32, P(vp)]),
        "pirip_hip_tx_destroy": (i32, [vp]),
        "pirip_hip_tx_get_info": (i32, [vp, P(TxInfo)]),
        "pirip_hip_tx_set_tones": (i32, [vp, vp, i32]),
        "pirip_hip_tx_set_gaps": (i32, [vp, vp, vp]),
        "pirip_hip_tx_reset": (i32, [vp, vp]),
        "pirip_hip_tx_max_syms": (i64, [vp, i32]),
        "pirip_hip_tx_frame": (i32, [vp, vp, sz, vp, i32, vp, sz, i64, vp, vp, sz, vp]),
        "pirip_hip_tx_modulate": (i32, [vp, vp, sz, vp, i64, i32, vp, sz, f32, f32, u64, vp]),
        "pirip_hip_tx_records_to_iq": (i32, [vp, vp, sz, vp, i32, i64, i32, vp, sz, f32, f32, u64, vp, vp]),
        "pirip_hip_tx_repeat_max_records": (i32, [vp, i32]),
        "pirip_hip_tx_repeat_records": (i32, [vp, vp, sz, vp, sz, vp, i32, i32, vp, sz, i32, vp, vp]),
        # section J: multiplexer
        "pirip_hip_mux_create": (i32, [i32, i32, i32, f32, i32, i32, i32, vp, vp, vp, i32, P(vp)]),
        "pirip_hip_mux_destroy": (i32, [vp]),
        "pirip_hip_mux_get_info": (i32, [vp, P(MuxInfo)]),
        "pirip_hip_mux_taps": (i32, [vp, vp, P(i32)]),
        "pirip_hip_mux_nout": (i64, [vp, i64]),
        "pirip_hip_mux_batch": (i32, [vp, vp, sz, i64, i64, vp, sz, vp]),
        # section K: streaming transmitter
        "pirip_hip_txs_create": (i32, [vp, vp, i64, i64, P(vp)]),
        "pirip_hip_txs_destroy": (i32, [vp]),
        "pirip_hip_txs_get_info": (i32, [vp, P(TxsInfo)]),
        "pirip_hip_txs_send": (i32, [vp, vp, sz, vp, i32, vp, vp]),
        "pirip_hip_txs_process": (i32, [vp, vp, sz, vp, vp]),
        "pirip_hip_txs_get_counters": (i32, [vp, vp, vp, vp, vp]),
        "pirip_hip_txs_reset": (i32, [vp, vp]),
        # section L: test-frame counter
        "pirip_hip_tbits_create": (i32, [i32, f32, vp, i32, i32, P(vp)]),
        "pirip_hip_tbits_destroy": (i32, [vp]),
        "pirip_hip_tbits_push": (i32, [vp, vp, sz, i32, i32, vp, i64, vp]),
        "pirip_hip_tbits_get_counters": (i32, [vp, vp, vp, vp, vp]),
        "pirip_hip_tbits_counters_device": (i32, [vp, P(vp)]),
        "pirip_hip_tbits_reset": (i32, [vp, vp]),
        "pirip_hip_tbits_testframe_payload": (i32, [i32, vp]),
        "pirip_hip_tbits_set_payload": (i32, [vp, i32, vp]),
        "pirip_hip_tbits_push_records": (i32, [vp, vp, sz, vp, sz, vp, sz, vp, i32, vp]),
        "pirip_hip_tbits_get_record_counters": (i32, [vp, vp, vp, vp, vp, vp]),
        # section M: streaming repeater
        "pirip_hip_rpt_create": (i32, [vp, vp, vp, i32, vp, i32, i32, i32, i32, i32, P(vp)]),
        "pirip_hip_rpt_destroy": (i32, [vp]),
        "pirip_hip_rpt_get_info": (i32, [vp, P(RptInfo)]),
        "pirip_hip_rpt_push_records": (i32, [vp, vp, sz, vp, sz, vp, i32, vp, sz, vp]),
        "pirip_hip_rpt_process": (i32, [vp, vp, sz, vp]),
        "pirip_hip_rpt_push": (i32, [vp, vp, sz, vp, sz, vp]),
        "pirip_hip_rpt_records": (i32, [vp] + [P(vp), P(sz)] * 3 + [P(vp)]),
        "pirip_hip_rpt_offered": (i32, [vp, P(vp), P(sz), P(vp)]),
        "pirip_hip_rpt_get_counters": (i32, [vp] + [vp] * 7),
        "pirip_hip_rpt_reset": (i32, [vp, vp]),
        # section N: ping terminal
        "pirip_hip_ping_create": (i32, [vp, vp, vp, P(PingConfig), P(vp)]),
        "pirip_hip_ping_destroy": (i32, [vp]),
        "pirip_hip_ping_get_info": (i32, [vp, P(PingInfo)]),
        "pirip_hip_ping_push_records": (i32, [vp, vp, sz, vp, sz, vp, sz, vp, sz, vp, i32, vp, sz, vp]),
        "pirip_hip_ping_process": (i32, [vp, vp, sz, vp]),
        "pirip_hip_ping_push": (i32, [vp, vp, sz, vp, sz, vp]),
        "pirip_hip_ping_records": (i32, [vp] + [P(vp), P(sz)] * 4 + [P(vp)]),
        "pirip_hip_ping_offered": (i32, [vp, P(vp), P(sz), P(vp)]),
        "pirip_hip_ping_get_counters": (i32, [vp] + [vp] * 9),
        "pirip_hip_ping_get_log": (i32, [vp, i32, vp, i32, P(i32)]),
        "pirip_hip_ping_reset": (i32, [vp, vp]),
        # section O: channel
        "pirip_hip_air_create": (i32, [i32, i32, i32, i32, i32, i32, vp, vp, u64, i32, P(vp)]),
        "pirip_hip_air_destroy": (i32, [vp]),
        "pirip_hip_air_get_info": (i32, [vp, P(AirInfo)]),
        "pirip_hip_air_set_sigma": (i32, [vp, vp, vp]),
        "pirip_hip_air_push": (i32, [vp, vp, sz, i64, vp, sz, vp]),
        "pirip_hip_air_reset": (i32, [vp, i64, vp]),
        "pirip_hip_air_create_ex": (i32, [i32, i32, i32, i32, i32, i32, vp, vp, u64, C.c_int32, i32, P(vp)]),
        "pirip_hip_air_interp_table": (i32, [vp, P(i32), P(i32)]),
        "pirip_hip_air_get_drift": (i32, [vp, P(C.c_int32), P(i64)]),
        "pirip_hip_air_reset_drift": (i32, [vp, i64, i64, vp]),
        "pirip_hip_air_create_fade": (i32, [i32, i32, i32, i32, i32, i32, vp, i32, vp, vp, u64, C.c_int32, i32, P(vp)]),
        "pirip_hip_air_fade_table": (i32, [i32, u64, P(AirFade), vp, vp, P(f32), P(f32)]),
        # section P: band monitor
        "pirip_hip_spec_create": (i32, [i32, i32, i32, i32, i32, i32, i32, vp, i32, P(vp)]),
        "pirip_hip_spec_destroy": (i32, [vp]),
        "pirip_hip_spec_get_info": (i32, [vp, P(SpecInfo)]),
        "pirip_hip_spec_window": (i32, [i32, vp]),
        "pirip_hip_spec_band_bins": (i32, [vp, i32, P(C.c_int32), P(C.c_int32)]),
        "pirip_hip_spec_nrows": (i64, [vp, i64]),
        "pirip_hip_spec_push": (i32, [vp, vp, sz, i64, vp, sz, sz, vp, sz, vp]),
        "pirip_hip_spec_reset": (i32, [vp, vp]),
        # section Q: diversity receiver
        "pirip_hip_div_create": (i32, [vp, P(DivConfig), P(vp)]),
        "pirip_hip_div_destroy": (i32, [vp]),
        "pirip_hip_div_get_info": (i32, [vp, P(DivInfo)]),
        "pirip_hip_div_reset": (i32, [vp, vp]),
        "pirip_hip_div_collect": (i32, [vp, vp, sz, vp, sz, vp, sz, vp, i32, vp]),
        "pirip_hip_div_push_candidates": (i32, [vp, vp, vp, vp, vp, i32, vp, vp]),
        "pirip_hip_div_flush": (i32, [vp, vp]),
        "pirip_hip_div_last": (i32, [vp, P(vp), P(sz), P(vp), P(sz), P(vp)]),
        "pirip_hip_div_get_log": (i32, [vp, i32, vp, vp, i32, P(i32)]),
        "pirip_hip_div_get_counters": (i32, [vp] + [vp] * 6),
        "pirip_hip_div_get_combined": (i32, [vp, i32, i32, vp]),
        # section R: packet link
        "pirip_hip_pkt_create": (i32, [vp, vp, vp, P(PktConfig), P(vp)]),
        "pirip_hip_pkt_destroy": (i32, [vp]),
        "pirip_hip_pkt_get_info": (i32, [vp, P(PktInfo)]),
        "pirip_hip_pkt_send": (i32, [vp, vp, sz, sz, vp, i32, vp, vp, vp, vp]),
        "pirip_hip_pkt_push_records": (i32, [vp, vp, sz, vp, sz, vp, i32, vp, sz, vp]),
        "pirip_hip_pkt_process": (i32, [vp, vp, sz, vp]),
        "pirip_hip_pkt_push": (i32, [vp, vp, sz, vp, sz, vp]),
        "pirip_hip_pkt_records": (i32, [vp] + [P(vp), P(sz)] * 2 + [P(vp)]),
        "pirip_hip_pkt_offered": (i32, [vp, P(vp), P(sz), P(vp)]),
        "pirip_hip_pkt_get_counters": (i32, [vp] + [vp] * 12),
        "pirip_hip_pkt_get_packets": (i32, [vp, i32, vp, vp, i32, P(i32)]),
        "pirip_hip_pkt_reset": (i32, [vp, vp]),
        "pirip_hip_pkt_create_fec": (i32, [vp, vp, vp, P(PktConfig), P(PktFecConfig), P(vp)]),
        "pirip_hip_pkt_get_fec_info": (i32, [vp, P(PktFecInfo)]),
        "pirip_hip_pkt_get_fec_counters": (i32, [vp] + [vp] * 4),
        # section S: ARQ sessions
        "pirip_hip_arq_create": (i32, [vp, P(ArqConfig), vp, P(vp)]),
        "pirip_hip_arq_destroy": (i32, [vp]),
        "pirip_hip_arq_get_info": (i32, [vp, P(ArqInfo)]),
        "pirip_hip_arq_submit": (i32, [vp, vp, sz, sz, vp, i32, vp, vp, vp]),
        "pirip_hip_arq_push_records": (i32, [vp, vp, sz, vp, sz, vp, i32, vp, sz, vp]),
        "pirip_hip_arq_process": (i32, [vp, vp, sz, vp]),
        "pirip_hip_arq_push": (i32, [vp, vp, sz, vp, sz, vp]),
        "pirip_hip_arq_get_counters": (i32, [vp] + [vp] * 19),
        "pirip_hip_arq_get_delivered": (i32, [vp, i32, vp, vp, i32, P(i32)]),
        "pirip_hip_arq_get_state": (i32, [vp, i32, P(i64), P(i64), P(i64), P(i64), P(C.c_uint32), P(i32)]),
        "pirip_hip_arq_reset": (i32, [vp, vp]),
        # section T: medium access
        "pirip_hip_mac_create": (i32, [vp, P(MacConfig), vp, P(vp)]),
        "pirip_hip_mac_destroy": (i32, [vp]),
        "pirip_hip_mac_get_info": (i32, [vp, P(MacInfo)]),
        "pirip_hip_mac_set_stats": (i32, [vp, vp, sz]),
        "pirip_hip_mac_stats": (i32, [vp, P(vp), P(sz)]),
        "pirip_hip_mac_get_counters": (i32, [vp] + [vp] * 8),
        "pirip_hip_mac_get_state": (i32, [vp, i32, P(i32), P(i32), P(i32), P(i32), P(i32)]),
        "pirip_hip_mac_reset": (i32, [vp, vp]),
        # the library itself
        "pirip_hip_find_code": (i32, [cs, cs, sz]),
        "pirip_hip_version": (cs, []),
        "pirip_hip_abi": (i32, [vp, vp, vp]),
        "pirip_hip_abi_check": (i32, [i32, i32, sz]),
        "pirip_hip_kernel_source_hash": (cs, []),
        "pirip_hip_strerror": (cs, [i32]),
        "pirip_hip_device_count": (i32, []),
        "pirip_hip_selftest_sqrt": (i32, [P(u64)]),
        "pirip_hip_selftest_div": (i32, [P(u64)]),
        "pirip_hip_selftest_atan2": (i32, [vp, vp, vp, i32]),
    }


# C name -> (restype, argtypes): every prototype of include/pirip_hip.h, in the header's order
SIGNATURES = _signatures()


def lib_path():
    return _LIB


def build(verbose=False):
    """Compile libpirip_hip.so + tools in-tree (hipcc --offload-arch=gfx950)."""
    cmd = ["make", "-C", os.path.join(_HERE, "csrc"), "-j8"]
    if not verbose:
        cmd.append("-s")
    subprocess.check_call(cmd)


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB):
        raise PiripError(f"{_LIB} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                         "(there is no fallback implementation)")
    # PyTorch wheels bundle their own HIP runtime (torch/lib/libamdhip64.so). Two HIP runtimes in
    # one process do not share the device, so when torch is importable load it FIRST: the
    # dynamic loader then satisfies libpirip_hip.so's libamdhip64 dependency from the copy that
    # is already mapped, and device pointers / streams from torch are valid in our calls.
    if os.environ.get("PIRIP_NO_TORCH_PRELOAD") is None:
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    L = C.CDLL(_LIB)
    for name, (restype, argtypes) in SIGNATURES.items():
        try:
            fn = getattr(L, name)
        except AttributeError:
            raise PiripError(f"{_LIB} does not export {name} (include/pirip_hip.h declares it): rebuild the library") from None
        fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


def _chk(rc, what):
    if rc != 0:
        raise PiripError(f"{what}: {lib().pirip_hip_strerror(rc).decode()} ({rc})")


def _dev(x):
    """a device pointer: None / 0, an int, or anything with data_ptr() (a torch tensor)"""
    if x is None:
        return 0
    return int(x.data_ptr()) if hasattr(x, "data_ptr") else int(x)


def _hip_stream(stream):
    """stream=None: torch's current stream when torch is loaded, else the default stream"""
    if stream is not None:
        return int(stream)
    torch = sys.modules.get("torch")
    return int(torch.cuda.current_stream().cuda_stream) if torch is not None and torch.cuda.is_available() else 0


def device_count():
    return int(lib().pirip_hip_device_count())


def kernel_source_hash():
    """pirip_hip_kernel_source_hash: 16 hex digits that name the kernel sources the library was built from (profiles/hbm_traffic.json
    carries the hash its counters were taken on)."""
    return lib().pirip_hip_kernel_source_hash().decode()


def _mismatches(name):
    m = C.c_uint64(0)
    _chk(getattr(lib(), name)(C.byref(m)), name)
    return int(m.value)


def selftest_sqrt():
    """Mismatches of the wave kernel's correctly rounded square roots against (float)sqrt((double)x) over x = 0 and every
    float in [2^-96, FLT_MAX], counted on the device (pirip_hip_selftest_sqrt): (v_sqrt variant << 32) | rsq variant."""
    return _mismatches("pirip_hip_selftest_sqrt")


def selftest_div():
    """Mismatches of the fused hand-over's x / 3 and x / 50 (pirip_hip_selftest_div) against the device's IEEE quotient over their measured
    domains -- x / 3: every finite x >= 0, denormals included; x / 50: x = 0 and every float in [2^-125, FLT_MAX]:
    (count for / 50 << 32) | count for / 3."""
    return _mismatches("pirip_hip_selftest_div")


def selftest_atan2(d_y, d_x, d_out, n):
    """pirip_hip_selftest_atan2: the exact prologue's atan2f of n float pairs d_y, d_x into d_out (device pointers or tensors), on the
    default stream; the caller synchronises."""
    _chk(lib().pirip_hip_selftest_atan2(_dev(d_y), _dev(d_x), _dev(d_out), int(n)), "pirip_hip_selftest_atan2")


def recalled(**overrides):
    """pirip_hip_recalled_defaults() with the named fields replaced."""
    r = FskRecalled()
    lib().pirip_hip_recalled_defaults(C.byref(r))
    for k, v in overrides.items():
        if k not in dict(FskRecalled._fields_):
            raise KeyError(k)
        setattr(r, k, v)
    return r


def launch_first_tail_block(nblocks, streams_per_cu, streams_per_block, cus):
    """pirip_hip_launch_first_tail_block (no device): the first workgroup of a wave-kernel launch of `nblocks` that starts at the raised
    priority; nblocks: none does."""
    first = int(lib().pirip_hip_launch_first_tail_block(int(nblocks), int(streams_per_cu), int(streams_per_block), int(cus)))
    if first < 0:
        _chk(first, "pirip_hip_launch_first_tail_block")
    return first


class _Handle:
    """One object of the library: its C handle h (None once closed, or when create failed), the library L, and the object's life cycle.
    A class names its C prefix (_c: pirip_hip_<section>, whose _destroy and _get_info are its) and, where it has one, its info structure."""
    _c = None
    _Info = None
    L = h = None

    def _create(self, name, *args):
        """the create entry point `name`: args, then the handle out; reads self.info where the class has an info structure"""
        self.L = lib()
        h = C.c_void_p()
        _chk(getattr(self.L, name)(*args, C.byref(h)), name)
        self.h = h
        if self._Info is not None:
            self.info = self._Info()
            self._call(self._c + "_get_info", C.byref(self.info))

    def _ptr(self, name):
        """the handle for a call of `name`: a closed object raises here, before C sees a NULL"""
        if self.h is None:
            raise PiripError(f"{name}: this {type(self).__name__} is closed")
        return self.h

    def _call(self, name, *args):
        """name(h, *args), which returns a status (every measured call comes through here: one test, one C call, one compare)"""
        if self.h is None:
            self._ptr(name)
        rc = getattr(self.L, name)(self.h, *args)
        if rc != 0:
            _chk(rc, name)

    def _value(self, name, *args):
        """name(h, *args), which returns a value"""
        return getattr(self.L, name)(self._ptr(name), *args)

    def _taps(self):
        """the *_taps protocol: ask for the length, allocate, ask again"""
        n = C.c_int(0)
        self._call(self._c + "_taps", None, C.byref(n))
        t = np.zeros(n.value, dtype=np.float32)
        self._call(self._c + "_taps", t.ctypes.data, C.byref(n))
        return t

    def close(self):
        h, self.h = self.h, None
        if h is not None:
            getattr(self.L, self._c + "_destroy")(h)

    def __del__(self):
        try:       # never raises: at interpreter shutdown the library or this module may be gone before the object
            self.close()
        except Exception:
            pass


def _ptr_of(obj, name):
    """obj's handle for a call of `name`, NULL for no object"""
    return None if obj is None else obj._ptr(name)


class HipDemod(_Handle):
    """nstreams device-resident demodulators (pirip_hip_create; recalled=dict(field=value, ...): pirip_hip_create_recalled)."""
    _c, _Info = "pirip_hip", FskInfo

    def __init__(self, Fs, Rs, M, P=8, Nsym=50, est_min=0, est_max=0, mask=0, in_format=IN_CU8_FSKDEMOD,
                 nstreams=1, device=-1, recalled=None):
        self.params = FskParams(Fs, Rs, M, P, Nsym, est_min, est_max, 1 if mask else 0, mask if mask else 100, in_format)
        if recalled is None:
            self._create("pirip_hip_create", C.byref(self.params), nstreams, device)
        else:
            self._create("pirip_hip_create_recalled", C.byref(self.params), C.byref(globals()["recalled"](**recalled)), nstreams, device)
        self.nstreams = nstreams
        self.M, self.Nsym, self.Nbits, self.N = M, Nsym, self.info.Nbits, self.info.N

    def kernel(self):
        """'wave' / 'block' (a specialised instance), 'general', or 'exact' (PIRIP_KERNEL=exact: every frame in the CPU algorithm's own
        operation order, the on-device cross-check) -- pirip_hip_get_kernel."""
        k = self._value("pirip_hip_get_kernel")
        return "wave" if k == 2 else "block" if k == 3 else "exact" if k == 4 else "general"

    def kernel_name(self):
        """pirip_hip_get_kernel_name: the instance's template arguments / the general kernel's run-time shape."""
        buf = C.create_string_buffer(256)
        self._call("pirip_hip_get_kernel_name", buf, 256)
        return buf.value.decode()

    def reset(self, stream=0):
        self._call("pirip_hip_reset", stream)

    def max_frames_for(self, nsamp):
        return nsamp // (2 * self.N - self.info.nin_max) + 2          # (the shortest frame: N - the nin step)

    def demod_batch(self, d_in, in_stride, nsamp, d_bits=0, bits_stride=0, d_filt=0, filt_stride=0,
                    d_stats=0, stats_stride=0, d_nframes=0, d_consumed=0, max_frames=None, stream=0):
        """Raw device pointers (ints); enqueues on `stream`, does not synchronise."""
        if max_frames is None:
            max_frames = self.max_frames_for(nsamp)
        self._call("pirip_hip_demod_batch", d_in, in_stride, nsamp, d_bits, bits_stride, d_filt, filt_stride,
                   d_stats, stats_stride, d_nframes, d_consumed, max_frames, stream)

    def demod_capture(self, d_in, nsamp, d_bits, d_filt=0, d_stats=0, max_frames=None, stream=0):
        """One long capture on the handle's stream slots (pirip_hip_demod_capture): raw device pointers; synchronises.
        Returns (nframes, consumed, report dict)."""
        if max_frames is None:
            max_frames = self.max_frames_for(nsamp)
        nf, cons, rep = C.c_int64(0), C.c_int64(0), CaptureReport()
        self._call("pirip_hip_demod_capture", d_in, nsamp, d_bits, d_filt, d_stats, max_frames, C.byref(nf), C.byref(cons), C.byref(rep),
                   stream)
        return nf.value, cons.value, {k: getattr(rep, k) for k, _ in CaptureReport._fields_}

    def demod_host(self, buf, want_filt=True):
        """numpy buffer [n, 2] in the configured format -> dict (stream 0; uploads/downloads)."""
        buf = np.ascontiguousarray(buf)
        nsamp = buf.shape[0]
        maxf = self.max_frames_for(nsamp)
        fb = (self.Nbits + 7) // 8 if getattr(self, "packed", False) else self.Nbits
        bits = np.zeros((maxf, fb), dtype=np.uint8)
        filt = np.zeros((maxf, self.M * self.Nsym), dtype=np.float32)
        st = np.zeros((maxf, STATS_PER_FRAME), dtype=np.float32)
        nf, cons = C.c_int64(0), C.c_int64(0)
        self._call("pirip_hip_demod_host", buf.ctypes.data, nsamp, bits.ctypes.data, filt.ctypes.data if want_filt else None,
                   st.ctypes.data, maxf, C.byref(nf), C.byref(cons))
        n = nf.value
        return {"nframes": n, "consumed": cons.value, "bits": bits[:n], "rx_filt": filt[:n] if want_filt else None,
                "stats": st[:n]}

    def set_bit_packing(self, packed=True):
        """d_bits becomes ceil(Nbits/8) bytes per frame, MSB first (strides in packed bytes)."""
        self._call("pirip_hip_set_bit_packing", 1 if packed else 0)
        self.packed = bool(packed)

    def set_exact_first_frame(self, enable=True):
        """pirip_hip_set_exact_first_frame: the prologue that demodulates a created stream's first frame in the CPU restatement's own
        operation order where P == Ts (default on); off: frame 0 comes from the handle's kernel like every other frame (A/B runs)."""
        self._call("pirip_hip_set_exact_first_frame", 1 if enable else 0)

    def set_estimator_band_only(self, enable=True):
        """Opt-in: Sf is maintained only for the FFT bins the peak search can read (include/pirip_hip.h); outputs unchanged."""
        self._call("pirip_hip_set_estimator_band_only", 1 if enable else 0)

    def set_launch_tail_first(self, enable=True):
        """pirip_hip_set_launch_tail_first: the workgroups of a wave-kernel launch's last residency start at a raised wave priority
        (default on); outputs unchanged."""
        self._call("pirip_hip_set_launch_tail_first", 1 if enable else 0)

    def launch_resident_blocks(self):
        """pirip_hip_get_launch_resident_blocks: workgroups of the handle's wave instance that its device holds at once (0: another kernel)."""
        return int(self._value("pirip_hip_get_launch_resident_blocks"))

    def set_freq_est_limits(self, est_min, est_max):
        """fsk_set_freq_est_limits() on the live handle; returns the status code (PIRIP_OK = 0) instead of raising."""
        return int(self._value("pirip_hip_set_freq_est_limits", int(est_min), int(est_max)))

    def set_burst_mode(self, enable=True):
        self._call("pirip_hip_set_burst_mode", 1 if enable else 0)

    def enable_eye(self, enable=True):
        """MODEM_STATS.rx_eye: keep the eye traces of each stream's latest frame (moves the handle to the general kernel, resets state)."""
        self._call("pirip_hip_enable_eye", 1 if enable else 0)

    def eye(self, s=0, normalise=True):
        out = np.zeros((8, 160), dtype=np.float32)
        ntr, npt = C.c_int(0), C.c_int(0)
        self._call("pirip_hip_get_eye", s, 1 if normalise else 0, out.ctypes.data, C.byref(ntr), C.byref(npt))
        return out[:ntr.value, :npt.value].copy()

    def get_Sf(self, s=0):
        out = np.zeros(self.info.Ndft, dtype=np.float32)
        self._call("pirip_hip_get_Sf", s, out.ctypes.data)
        return out

    def stream_state(self, s=0):
        """pirip_hip_get_stream_state: the StreamState of stream s after the last call. Synchronises."""
        st = StreamState()
        self._call("pirip_hip_get_stream_state", s, C.byref(st))
        return st


class HipDecim(_Handle):
    """csdr convert_u8_f | fir_decimate_cc D | [convert_f_s16] as one device stage."""
    _c = "pirip_hip_decim"

    def __init__(self, D, transition_bw=0.05, out_s16=True, device=-1):
        self._create("pirip_hip_decim_create", D, transition_bw, 1 if out_s16 else 0, device)
        self.D, self.out_s16 = D, out_s16

    def taps(self):
        return self._taps()

    def nout(self, n_in):
        return int(self._value("pirip_hip_decim_nout", n_in))

    def set_arith(self, mode):
        """0 exact (default: the scalar csdr loop bit for bit), 1 fused accumulate, 2 affine map pulled out of the sum (opt-in measurements)"""
        self._call("pirip_hip_decim_set_arith", int(mode))

    def get_arith(self):
        """pirip_hip_decim_get_arith: the tap-loop arithmetic in use, as set_arith's mode (or PIRIP_DECIM_FMA at create)"""
        return int(self._value("pirip_hip_decim_get_arith"))

    def batch(self, d_in, in_stride, n_in, d_out, out_stride, nstreams, stream=0):
        self._call("pirip_hip_decim_batch", d_in, in_stride, n_in, d_out, out_stride, nstreams, stream)


class HipChan(_Handle):
    """Channelizer (include/pirip_hip.h section H): channel c = csdr shift_addition_cc (-offsets[c]/Fs) | fir_decimate_cc D of capture
    inputs[c] (all 0 when inputs is None), for every channel of every capture in one pass over the u8 IQ. out_s16: interleaved s16 IQ out
    (convert_f_s16), else complex float."""
    _c, _Info = "pirip_hip_chan", ChanInfo

    def __init__(self, Fs, D, offsets, inputs=None, transition_bw=0.05, out_s16=False, device=-1):
        off = np.ascontiguousarray(offsets, dtype=np.int32).reshape(-1)
        inp = np.zeros(off.size, dtype=np.int32) if inputs is None else np.ascontiguousarray(inputs, dtype=np.int32).reshape(-1)
        if inp.size != off.size:
            raise ValueError("inputs and offsets must have the same length")
        ninputs = int(inp.max()) + 1 if inp.size else 1
        self._create("pirip_hip_chan_create", int(Fs), int(D), transition_bw, 1 if out_s16 else 0, ninputs, int(off.size),
                     inp.ctypes.data if inp.size else None, off.ctypes.data if off.size else None, device)
        self.Fs, self.D, self.out_s16 = int(Fs), int(D), bool(out_s16)
        self.offsets, self.inputs = off.copy(), inp.copy()
        self.ninputs, self.nchan, self.Lp = self.info.ninputs, self.info.nchan, self.info.ntaps_padded
        self.bytes_per_sample = 4 if out_s16 else 8

    def taps(self):
        """the prototype low-pass h (section B's taps for the same D / transition_bw, unpadded)"""
        return self._taps()

    def nout(self, n_in):
        return int(self._value("pirip_hip_chan_nout", int(n_in)))

    def batch(self, d_in, in_stride, n_in, d_out, out_stride, t0=0, stream=0):
        """capture i at d_in + i * in_stride (n_in u8 IQ samples, the first at absolute index t0) -> channel c at d_out + c * out_stride
        (nout(n_in) samples); raw device pointers, enqueued on `stream`, does not synchronise"""
        self._call("pirip_hip_chan_batch", d_in, in_stride, int(n_in), int(t0), d_out, out_stride, stream)


TX_CARRIER_OFF = 0xFF


class HipTx(_Handle):
    """nstreams FSK_LDPC transmitters (include/pirip_hip.h section I): records of rpitx_fsk --code's stdin protocol -> channel symbols ->
    continuous-phase M-FSK IQ. f1: one first-tone frequency for all streams or one per stream (Hz); lead / gap: carrier-off symbols in
    front of a stream's first record and for each of its `2` records (scalars or one per stream)."""
    _c, _Info = "pirip_hip_tx", TxInfo

    def __init__(self, code_path, Fs, Rs, M, nstreams=1, f1=None, shift=None, lead=0, gap=0, device=-1):
        self._create("pirip_hip_tx_create", code_path.encode(), int(Fs), int(Rs), int(M), int(nstreams), device)
        self.Fs, self.Rs, self.M, self.Ts, self.nstreams = int(Fs), int(Rs), int(M), self.info.Ts, int(nstreams)
        self.k, self.data_bytes, self.record_bytes = self.info.k, self.info.data_bytes, 1 + self.info.data_bytes
        self.bits_per_frame, self.frame_syms, self.preamble_syms = self.info.bits_per_frame, self.info.frame_syms, self.info.preamble_syms
        self.bps = 1 if M == 2 else 2
        if f1 is not None:
            self.set_tones(f1, shift if shift is not None else Rs)
        self.set_gaps(lead, gap)

    def _per_stream(self, v):
        a = np.ascontiguousarray(v, dtype=np.int32).reshape(-1)
        if a.size == 1:
            a = np.full(self.nstreams, int(a[0]), dtype=np.int32)
        if a.size != self.nstreams:
            raise ValueError("one value, or one per stream")
        return a

    def set_tones(self, f1, shift):
        a = self._per_stream(f1)
        self._call("pirip_hip_tx_set_tones", a.ctypes.data, int(shift))

    def set_gaps(self, lead=0, gap=0):
        a, b = self._per_stream(lead), self._per_stream(gap)
        self._call("pirip_hip_tx_set_gaps", a.ctypes.data, b.ctypes.data)

    def reset(self, stream=0):
        self._call("pirip_hip_tx_reset", stream)

    def max_syms(self, max_rec):
        return int(self._value("pirip_hip_tx_max_syms", int(max_rec)))

    def frame(self, d_records, rec_stride, max_rec, d_syms, sym_stride, max_syms, d_nrec=0, d_nsym=0, d_bits=0, bits_stride=0, stream=0):
        """records -> symbol rows (and the framer's bits); raw device pointers, enqueued on `stream`, does not synchronise"""
        self._call("pirip_hip_tx_frame", d_records, rec_stride, d_nrec, int(max_rec), d_syms, sym_stride, int(max_syms), d_nsym,
                   d_bits, bits_stride, stream)

    def modulate(self, d_syms, sym_stride, nsym, d_out, out_stride, out_format=IN_CU8_FSKDEMOD, d_nsym=0, amp=32.0, sigma=0.0, seed=1,
                 stream=0):
        """nsym symbol times (nsym * Ts samples) per stream -> IQ rows; continues where the previous call stopped"""
        self._call("pirip_hip_tx_modulate", d_syms, sym_stride, d_nsym, int(nsym), out_format, d_out, out_stride, amp, sigma, seed, stream)

    def repeat_max_records(self, ncalls):
        return int(self._value("pirip_hip_tx_repeat_max_records", int(ncalls)))

    def repeat_records(self, d_status, status_stride, d_payload, payload_stride, ncalls, source_byte, d_records, rec_stride, max_rec,
                       d_ncalls=0, d_nrec=0, stream=0):
        """receiver records (HipLdpc.chain_batch's status / payload rows) -> Tx records by frame_repeater's state machine, on the device;
        a burst still being received waits in the handle for the call in which it ends"""
        self._call("pirip_hip_tx_repeat_records", d_status, status_stride, d_payload, payload_stride, d_ncalls, int(ncalls),
                   int(source_byte), d_records, rec_stride, int(max_rec), d_nrec, stream)

    def records_to_iq(self, d_records, rec_stride, max_rec, nsym, d_out, out_stride, out_format=IN_CU8_FSKDEMOD, d_nrec=0, d_nsym=0,
                      amp=32.0, sigma=0.0, seed=1, stream=0):
        self._call("pirip_hip_tx_records_to_iq", d_records, rec_stride, d_nrec, int(max_rec), int(nsym), out_format, d_out, out_stride,
                   amp, sigma, seed, d_nsym, stream)


MUX_FIR, MUX_LINEAR = 0, 1


class HipMux(_Handle):
    """Multiplexer (include/pirip_hip.h section J), the channelizer's mirror image: channel c (complex float at Fs / D) is interpolated
    by D, moved to offsets[c] Hz, scaled by gains[c] (all 1 when gains is None) and added to wideband stream outputs[c] (all 0 when
    outputs is None; noutputs: more streams than the largest index, the others empty). kind: MUX_FIR (D times section B's low-pass) or
    MUX_LINEAR; out_format: IN_CU8_CSDR (u8 IQ) or IN_CF32."""
    _c, _Info = "pirip_hip_mux", MuxInfo

    def __init__(self, Fs, D, offsets, outputs=None, gains=None, kind=MUX_FIR, transition_bw=0.05, out_format=IN_CU8_CSDR, device=-1,
                 noutputs=None):
        off = np.ascontiguousarray(offsets, dtype=np.int32).reshape(-1)
        outp = np.zeros(off.size, dtype=np.int32) if outputs is None else np.ascontiguousarray(outputs, dtype=np.int32).reshape(-1)
        g = None if gains is None else np.ascontiguousarray(gains, dtype=np.float32).reshape(-1)
        if outp.size != off.size or (g is not None and g.size != off.size):
            raise ValueError("outputs, gains and offsets must have the same length")
        if noutputs is None:
            noutputs = int(outp.max()) + 1 if outp.size else 1
        self._create("pirip_hip_mux_create", int(Fs), int(D), int(kind), transition_bw, int(out_format), int(noutputs), int(off.size),
                     outp.ctypes.data if outp.size else None, off.ctypes.data if off.size else None,
                     g.ctypes.data if g is not None and g.size else None, device)
        self.Fs, self.D, self.kind, self.out_format = int(Fs), int(D), int(kind), int(out_format)
        self.offsets, self.outputs = off.copy(), outp.copy()
        self.gains = np.ones(off.size, dtype=np.float32) if g is None else g.copy()
        self.Q, self.ntaps, self.ntaps_padded = self.info.Q, self.info.ntaps, self.info.ntaps_padded
        self.nchan, self.noutputs = self.info.nchan, self.info.noutputs
        self.bytes_per_sample = 8 if out_format == IN_CF32 else 2

    def taps(self):
        """the prototype h (ntaps, unpadded)"""
        return self._taps()

    def nout(self, n_in):
        return int(self._value("pirip_hip_mux_nout", int(n_in)))

    def batch(self, d_in, in_stride, n_in, d_out, out_stride, m0=0, stream=0):
        """channel c at d_in + c * in_stride (n_in complex floats, the first at absolute index m0) -> output i at d_out + i * out_stride
        (nout(n_in) samples, the first at absolute index (m0 + Q - 1) D); raw device pointers, enqueued on `stream`, does not synchronise"""
        self._call("pirip_hip_mux_batch", d_in, in_stride, int(n_in), int(m0), d_out, out_stride, stream)


class HipTxStream(_Handle):
    """Streaming transmitter (include/pirip_hip.h section K): every channel of HipTx `tx` has a symbol queue on the device, and each
    process() turns the next S = block / (D Ts) symbols of every queue into `block` wideband samples per output of HipMux `mux`, with no
    modem-rate IQ in between. queue_syms: each queue's capacity in symbols (>= S). Both handles must outlive the stream."""
    _c, _Info = "pirip_hip_txs", TxsInfo

    def __init__(self, tx, mux, block, queue_syms):
        self.tx, self.mux = tx, mux
        self._create("pirip_hip_txs_create", tx._ptr("pirip_hip_txs_create"), mux._ptr("pirip_hip_txs_create"), int(block), int(queue_syms))
        self.block, self.queue_syms, self.S, self.H = self.info.block, self.info.queue_syms, self.info.S, self.info.H
        self.nchan, self.noutputs, self.bytes_per_sample = self.info.nchan, self.info.noutputs, mux.bytes_per_sample

    def send(self, d_records, rec_stride, max_rec, d_nrec=0, d_taken=0, stream=0):
        """offer every channel its records (HipTx.frame's format); per channel all or nothing, d_taken[s] = records taken. Raw device
        pointers, enqueued on `stream`."""
        self._call("pirip_hip_txs_send", d_records, rec_stride, d_nrec, int(max_rec), d_taken, stream)

    def process(self, d_out, out_stride, d_sent=0, stream=0):
        """one block: output i gets `block` samples at d_out + i * out_stride; d_sent[s] = symbols dequeued. Does not synchronise."""
        self._call("pirip_hip_txs_process", d_out, out_stride, d_sent, stream)

    def counters(self):
        """dict of int64[nchan]: queued, sent, underrun, refused -- synchronises."""
        out = {k: np.zeros(self.nchan, dtype=np.int64) for k in ("queued", "sent", "underrun", "refused")}
        self._call("pirip_hip_txs_get_counters", *(a.ctypes.data for a in out.values()))
        return out

    def reset(self, stream=0):
        self._call("pirip_hip_txs_reset", stream)


def testframe_payload(k):
    """The --testframes payload of a code with k data bits, packed MSB first: uint8[k / 8] (pirip_hip_tbits_testframe_payload; no device)."""
    out = np.zeros(max(int(k) // 8, 1), dtype=np.uint8)
    _chk(lib().pirip_hip_tbits_testframe_payload(int(k), out.ctypes.data), "pirip_hip_tbits_testframe_payload")
    return out


class HipTestBits(_Handle):
    """Test-frame counter (include/pirip_hip.h section L): fsk_put_test_bits [-f framesize] [-t valid_thresh] for nstreams streams, counted
    on the device. frame: None for the tool's own frame, else framesize values 0 / 1. push() takes the demodulator's bit rows,
    push_records() the FSK_LDPC receiver's records (rtl_fsk --testframes' ecdd, tallied)."""
    _c = "pirip_hip_tbits"

    def __init__(self, framesize=100, valid_thresh=0.1, frame=None, nstreams=1, device=-1):
        fb = None
        if frame is not None:
            fb = np.ascontiguousarray(frame, dtype=np.uint8).reshape(-1)
            if fb.size != framesize:
                raise ValueError("frame must hold framesize bits")
        self._create("pirip_hip_tbits_create", int(framesize), float(valid_thresh), None if fb is None else fb.ctypes.data, int(nstreams),
                     device)
        self.framesize, self.valid_thresh, self.nstreams, self.data_bytes = int(framesize), float(valid_thresh), int(nstreams), 0

    def push(self, bits, nframes=None, row_bits=None, packed=False, stream=None, max_frames=None, bits_stride=None):
        """bits: a uint8 tensor [nstreams, max_frames, row bytes] (the last two dimensions contiguous) or a raw device pointer with
        max_frames and bits_stride (bytes per stream) given; nframes: int32 tensor / pointer [nstreams] or None (every row counts);
        row_bits: bits per row (default: the row's bytes, unpacked). Enqueued on `stream` (None: torch's current stream); no synchronisation."""
        if hasattr(bits, "data_ptr") and hasattr(bits, "shape"):
            if bits.dim() != 3 or bits.shape[0] != self.nstreams or bits.element_size() != 1:
                raise ValueError("bits: uint8 [nstreams, max_frames, row bytes]")
            rb = int(bits.shape[2])
            if row_bits is None:
                if packed:
                    raise ValueError("packed rows need row_bits")
                row_bits = rb
            need = (int(row_bits) + 7) // 8 if packed else int(row_bits)
            if rb != need or (bits.shape[1] > 1 and bits.stride(1) != rb) or bits.stride(2) != 1:
                raise ValueError("bits: rows of exactly row_bits bits, one after the other")
            max_frames = int(bits.shape[1]) if max_frames is None else int(max_frames)
            bits_stride = int(bits.stride(0)) if bits_stride is None else int(bits_stride)
        elif max_frames is None or bits_stride is None or row_bits is None:
            raise ValueError("a raw pointer needs row_bits, max_frames and bits_stride")
        self._call("pirip_hip_tbits_push", _dev(bits), int(bits_stride), int(row_bits), 1 if packed else 0, _dev(nframes), int(max_frames),
                   _hip_stream(stream))

    def set_payload(self, data_bytes, payload=None):
        """what push_records compares with: data_bytes bytes, None = testframe_payload(8 * data_bytes)"""
        p = None if payload is None else np.ascontiguousarray(payload, dtype=np.uint8).reshape(-1)
        if p is not None and p.size != data_bytes:
            raise ValueError("payload must hold data_bytes bytes")
        self._call("pirip_hip_tbits_set_payload", int(data_bytes), None if p is None else p.ctypes.data)
        self.data_bytes = int(data_bytes)

    def push_records(self, status, payload, info, ncalls=None, max_calls=None, status_stride=None, payload_stride=None, info_stride=None,
                     stream=None):
        """the records HipLdpc.chain_batch / HipRx.process wrote: status uint8 [nstreams, max_calls], payload uint8 [nstreams, max_calls,
        data_bytes], info int32 [nstreams, max_calls, LDPC_INFO_PER_CALL] as tensors (per-stream rows contiguous), or raw pointers with
        max_calls and the three strides (elements per stream); ncalls: int32 [nstreams] or None."""
        if hasattr(status, "shape"):
            max_calls = int(status.shape[1]) if max_calls is None else int(max_calls)
            status_stride = int(status.stride(0)) if status_stride is None else int(status_stride)
            payload_stride = int(payload.stride(0)) if payload_stride is None else int(payload_stride)
            info_stride = int(info.stride(0)) if info_stride is None else int(info_stride)
        elif None in (max_calls, status_stride, payload_stride, info_stride):
            raise ValueError("raw pointers need max_calls and the three strides")
        self._call("pirip_hip_tbits_push_records", _dev(status), status_stride, _dev(payload), payload_stride, _dev(info), info_stride,
                   _dev(ncalls), int(max_calls), _hip_stream(stream))

    def _read(self, name, names):
        out = {k: np.zeros(self.nstreams, dtype=np.int64) for k in names}
        self._call(name, *(out[k].ctypes.data for k in names))
        return out

    def counters(self):
        """dict of int64[nstreams]: packets, bits, errors (fsk_put_test_bits' packetcnt, bitcnt, biterr), pushed -- synchronises."""
        return self._read("pirip_hip_tbits_get_counters", ("packets", "bits", "errors", "pushed"))

    def counters_device(self):
        """device pointer of the int64 [nstreams][4] counters {packets, bits, errors, pushed}"""
        p = C.c_void_p()
        self._call("pirip_hip_tbits_counters_device", C.byref(p))
        return int(p.value)

    def record_counters(self):
        """dict of int64[nstreams]: frames (decoded), bits (payload bits compared), errors, frames_in_error, crc_ok -- synchronises."""
        return self._read("pirip_hip_tbits_get_record_counters", ("frames", "bits", "errors", "frames_in_error", "crc_ok"))

    def reset(self, stream=None):
        self._call("pirip_hip_tbits_reset", _hip_stream(stream))


class _Terminal(_Handle):
    """What the repeater and the ping terminal share: a receiver's block in, a transmitter stream's block out, the C names apart."""

    def process(self, out, out_stride, stream=None):
        """the block at rx.input() -> one block per output (needs rx)"""
        self._call(self._c + "_process", _dev(out), int(out_stride), _hip_stream(stream))

    def push(self, d_in, in_stride, out, out_stride, stream=None):
        """process() after copying the block from d_in (rows in_stride bytes apart) into rx's input"""
        self._call(self._c + "_push", _dev(d_in), int(in_stride), _dev(out), int(out_stride), _hip_stream(stream))

    def _records(self, rows):
        """<prefix>_records: a device pointer and a stride in elements for each of `rows`, then the pointer of nframes"""
        p = [C.c_void_p() for _ in range(len(rows) + 1)]
        st = [C.c_size_t(0) for _ in rows]
        self._call(self._c + "_records", *(C.byref(x) for pair in zip(p, st) for x in pair), C.byref(p[-1]))
        out = {"nframes": int(p[-1].value or 0)}
        for k, ptr, stride in zip(rows, p, st):
            out[k], out[k + "_stride"] = int(ptr.value or 0), int(stride.value)
        return out

    def offered(self):
        """(device pointer of the records offered in the last call, bytes per channel row, device pointer of the int32 [nchan] counts)"""
        p, n, st = C.c_void_p(), C.c_void_p(), C.c_size_t(0)
        self._call(self._c + "_offered", C.byref(p), C.byref(st), C.byref(n))
        return int(p.value), int(st.value), int(n.value)

    def reset(self, stream=None):
        self._call(self._c + "_reset", _hip_stream(stream))


class HipRepeater(_Terminal):
    """Streaming repeater (include/pirip_hip.h section M): one call per block from received FSK_LDPC records -- or, with a HipRx `rx`
    created with an ldpc, from wideband IQ -- to the repeated wideband IQ of HipTxStream `txs` (created on HipTx `tx`). route[c]: the
    transmit channel of receive channel c, negative = not repeated; source: byte 0 of every repeated frame; filter: None, or the byte 0
    of frames that are not repeated (the repeater's own); holdoff: calls a finished burst waits; max_burst: frames held per burst;
    pending: records of each transmit channel's pending ring (default: two bursts). The handles must outlive the repeater; pointer
    arguments take torch tensors or raw device pointers, streams default to torch's current stream."""
    _c, _Info = "pirip_hip_rpt", RptInfo

    def __init__(self, tx, txs, route, source, filter=None, holdoff=0, max_burst=100, pending=None, rx=None):
        self.rx, self.tx, self.txs = rx, tx, txs
        rt = np.ascontiguousarray(route, dtype=np.int32).reshape(-1)
        if pending is None:
            pending = 2 * (int(max_burst) + 1)
        name = "pirip_hip_rpt_create"
        self._create(name, _ptr_of(rx, name), tx._ptr(name), txs._ptr(name), int(rt.size), rt.ctypes.data, int(source),
                     -1 if filter is None else int(filter), int(holdoff), int(max_burst), int(pending))
        self.nrx, self.nchan, self.pending, self.rx_rows = self.info.nrx, self.info.nchan, self.info.pending_records, self.info.rx_rows
        self.data_bytes = tx.data_bytes

    def push_records(self, status, payload, out, out_stride, ncalls=None, max_calls=None, status_stride=None, payload_stride=None, stream=None):
        """status uint8 [nrx, max_calls], payload uint8 [nrx, max_calls, data_bytes] (tensors, per-channel rows contiguous; or raw
        pointers with max_calls and the strides), ncalls int32 [nrx] or None -> one block per output at out + i * out_stride."""
        if hasattr(status, "shape"):
            max_calls = int(status.shape[1]) if max_calls is None else int(max_calls)
            status_stride = int(status.stride(0)) if status_stride is None else int(status_stride)
            payload_stride = int(payload.stride(0)) if payload_stride is None else int(payload_stride)
        elif None in (max_calls, status_stride, payload_stride):
            raise ValueError("raw pointers need max_calls and the two strides")
        self._call("pirip_hip_rpt_push_records", _dev(status), status_stride, _dev(payload), payload_stride, _dev(ncalls), int(max_calls),
                   _dev(out), int(out_stride), _hip_stream(stream))

    def records(self):
        """dict of the last call's received records: device pointers status, payload, info, nframes and the strides in elements"""
        return self._records(("status", "payload", "info"))

    def counters(self):
        """dict of int64 arrays -- [nrx]: bursts_in, frames_in, filtered, unrouted; [nchan]: bursts_out, pending, dropped. Synchronises."""
        names = ("bursts_in", "frames_in", "filtered", "unrouted", "bursts_out", "pending", "dropped")
        out = {k: np.zeros(self.nrx if i < 4 else self.nchan, dtype=np.int64) for i, k in enumerate(names)}
        self._call("pirip_hip_rpt_get_counters", *(out[k].ctypes.data for k in names))
        return out


class HipPing(_Terminal):
    """Ping terminal (include/pirip_hip.h section N): per call the received FSK_LDPC records -- the caller's, or with a HipRx `rx` created
    with an ldpc those of the wideband block -- go through the filter into a log ring per receive channel, and on a schedule counted in
    calls a burst of `frames` test frames (source in byte 0, with seq the frame's number in byte 1) goes out through HipTxStream `txs`
    (created on HipTx `tx`). Without tx / txs the handle is a logger only and every call's out is None. first_call: the first due call
    per transmit channel (None: 0); period: calls between bursts; max_bursts: per channel, 0 = no limit; log_entries: entries of each
    ring; nin0: what the first demodulator call consumes (taken from rx where given). The handles must outlive the terminal; pointer
    arguments take torch tensors or raw device pointers, streams default to torch's current stream."""
    _c, _Info = "pirip_hip_ping", PingInfo

    RX_COUNTERS = ("frames", "filtered", "decoded", "crc_fail", "bit_errors", "lost")
    TX_COUNTERS = ("bursts_sent", "frames_sent", "skipped")

    def __init__(self, rx=None, tx=None, txs=None, nrx=None, source=1, filter=None, frames=3, seq=False, period=1, first_call=None, max_bursts=0,
                 log_entries=256, nin0=0):
        self.rx, self.tx, self.txs = rx, tx, txs
        if nrx is None:
            nrx = rx.nstreams if rx is not None else 0
        fc = None if first_call is None else np.ascontiguousarray(first_call, dtype=np.int32).reshape(-1)
        if fc is not None and tx is not None and fc.size != tx.nstreams:
            raise ValueError("first_call: one entry per transmit channel")
        cfg = PingConfig(int(nrx), int(source), -1 if filter is None else int(filter), int(frames), 1 if seq else 0, int(period),
                         None if fc is None else fc.ctypes.data_as(C.POINTER(C.c_int32)), int(max_bursts), int(log_entries), int(nin0))
        name = "pirip_hip_ping_create"
        self._create(name, _ptr_of(rx, name), _ptr_of(tx, name), _ptr_of(txs, name), C.byref(cfg))
        i = self.info
        self.nrx, self.nchan, self.rx_rows, self.data_bytes, self.log_entries, self.nin0 = i.nrx, i.nchan, i.rx_rows, i.data_bytes, i.log_entries, i.nin0
        self.frames = i.frames_per_burst

    def push_records(self, status, payload, info, stats, out=None, out_stride=0, ncalls=None, max_calls=None, status_stride=None,
                     payload_stride=None, info_stride=None, stats_stride=None, stream=None):
        """status uint8 [nrx, max_calls], payload uint8 [nrx, max_calls, data_bytes], info int32 [nrx, max_calls, 10], stats float32 [nrx,
        max_calls, 10] (tensors, per-channel rows contiguous; or raw pointers with max_calls and the strides in elements), ncalls int32
        [nrx] or None -> the log, and with tx one block per output at out + i * out_stride."""
        if hasattr(status, "shape"):
            max_calls = int(status.shape[1]) if max_calls is None else int(max_calls)
            status_stride = int(status.stride(0)) if status_stride is None else int(status_stride)
            payload_stride = int(payload.stride(0)) if payload_stride is None else int(payload_stride)
            info_stride = int(info.stride(0)) if info_stride is None else int(info_stride)
            stats_stride = int(stats.stride(0)) if stats_stride is None else int(stats_stride)
        elif None in (max_calls, status_stride, payload_stride, info_stride, stats_stride):
            raise ValueError("raw pointers need max_calls and the four strides")
        self._call("pirip_hip_ping_push_records", _dev(status), status_stride, _dev(payload), payload_stride, _dev(info), info_stride,
                   _dev(stats), stats_stride, _dev(ncalls), int(max_calls), _dev(out), int(out_stride), _hip_stream(stream))

    def process(self, out=None, out_stride=0, stream=None):
        """the block at rx.input() -> the log, and with tx one block per output (needs rx)"""
        super().process(out, out_stride, stream)

    def push(self, d_in, in_stride, out=None, out_stride=0, stream=None):
        """process() after copying the block from d_in (rows in_stride bytes apart) into rx's input"""
        super().push(d_in, in_stride, out, out_stride, stream)

    def records(self):
        """dict of the last call's rows: device pointers status, payload, info, stats, nframes and the strides in elements"""
        return self._records(("status", "payload", "info", "stats"))

    def counters(self):
        """dict of int64 arrays -- [nrx]: frames, filtered, decoded, crc_fail, bit_errors, lost; [nchan]: bursts_sent, frames_sent, skipped.
        Synchronises."""
        out = {k: np.zeros(self.nrx, dtype=np.int64) for k in self.RX_COUNTERS}
        out.update({k: np.zeros(self.nchan, dtype=np.int64) for k in self.TX_COUNTERS})
        self._call("pirip_hip_ping_get_counters", *(out[k].ctypes.data for k in self.RX_COUNTERS + self.TX_COUNTERS))
        return out

    def log(self, chan, max_entries=None):
        """the newest entries of receive channel chan, oldest first: numpy structured array of PING_ENTRY_DTYPE. Synchronises."""
        n = self.log_entries if max_entries is None else int(max_entries)
        out = np.zeros(max(n, 1), dtype=np.dtype(PING_ENTRY_DTYPE))
        assert out.dtype.itemsize == C.sizeof(PingEntry) == 40
        got = C.c_int(0)
        self._call("pirip_hip_ping_get_log", int(chan), out.ctypes.data, n, C.byref(got))
        return out[:got.value].copy()


class HipAir(_Handle):
    """Channel (include/pirip_hip.h section O): ntx transmitted wideband IQ streams onto nrx received ones. paths: AirPath entries, or
    tuples / dicts of (rx, tx, gain, delay, offset_hz) -- received stream rx hears transmitted stream tx scaled by the real gain, `delay`
    samples late and `offset_hz` Hz up; sigma: the noise per component of every received stream (a number, nrx numbers, or None for none),
    keyed by (seed, stream, absolute sample) as HipTx.modulate's; in_format / out_format: IN_CU8_CSDR or IN_CF32. The history of every
    transmitted stream stays on the device: any cutting of a stream into push() calls gives the same output. Pointer arguments take torch
    tensors or raw device pointers, streams default to torch's current stream.
    Two clocks that disagree: a sixth element or key `clock_ppb` (AirPathEx) is the clock offset of the path's transmitter
    in parts per billion, fast when positive; such a path is read through the interpolator and may slip max_slip whole samples, of its
    delay (fast: delay >= 8 + max_slip) or of the ring (slow). drift() says how many samples push() still takes, reset(n0, age=...)
    resumes at a clock age. Without a clock offset and with max_slip 0 the handle is pirip_hip_air_create's.
    Fading: fades is a list of AirFade, of tuples (path, doppler_hz, rice_k, key) or of dicts with those keys (rice_k and
    key default to 0) -- the path of that index gets a Rayleigh (rice_k 0) or Rician gain of that Doppler spread, a float in Hz that is
    rounded to whole millihertz. Without fades the handle is the one it was."""
    _c, _Info = "pirip_hip_air", AirInfo

    def __init__(self, Fs, paths, ntx, nrx, sigma=None, seed=1, in_format=IN_CU8_CSDR, out_format=IN_CU8_CSDR, device=-1, max_slip=0, fades=None):
        rows = []
        for p in paths:
            if isinstance(p, AirPathEx):
                rows.append((p.rx, p.tx, p.gain, p.delay, p.offset_hz, p.clock_ppb))
            elif isinstance(p, AirPath):
                rows.append((p.rx, p.tx, p.gain, p.delay, p.offset_hz))
            elif isinstance(p, dict):
                rows.append((p["rx"], p["tx"], p.get("gain", 1.0), p.get("delay", 0), p.get("offset_hz", 0)) +
                            ((p["clock_ppb"],) if "clock_ppb" in p else ()))
            else:
                rows.append(tuple(p))
        self.paths = rows
        sg = self._sigma(sigma, int(nrx))
        d_sg = None if sg is None else sg.ctypes.data
        common = (int(Fs), int(in_format), int(out_format), int(ntx), int(nrx), len(rows))
        self.fades = [air_fade(f) for f in fades or ()]
        if not self.fades and int(max_slip) == 0 and not any(len(p) > 5 and int(p[5]) for p in rows):
            arr = (AirPath * max(len(rows), 1))()
            for i, (rx, tx, gain, delay, off) in enumerate(p[:5] for p in rows):
                arr[i] = AirPath(int(rx), int(tx), int(delay), int(off), float(gain))
            self._create("pirip_hip_air_create", *common, C.addressof(arr) if rows else None, d_sg, int(seed), device)
        else:
            arr = (AirPathEx * max(len(rows), 1))()
            for i, p in enumerate(rows):
                arr[i] = AirPathEx(int(p[0]), int(p[1]), int(p[3]), int(p[4]), float(p[2]), int(p[5]) if len(p) > 5 else 0)
            d_arr = C.addressof(arr) if rows else None
            if self.fades:
                farr = (AirFade * len(self.fades))(*self.fades)
                self._create("pirip_hip_air_create_fade", *common, d_arr, len(self.fades), C.addressof(farr), d_sg, int(seed), int(max_slip),
                             device)
            else:
                self._create("pirip_hip_air_create_ex", *common, d_arr, d_sg, int(seed), int(max_slip), device)
        self.Fs, self.ntx, self.nrx, self.seed, self.max_delay = int(Fs), self.info.ntx, self.info.nrx, int(seed), self.info.max_delay
        self.in_format, self.out_format = int(in_format), int(out_format)
        self.in_bytes_per_sample = 8 if in_format == IN_CF32 else 2
        self.out_bytes_per_sample = 8 if out_format == IN_CF32 else 2

    @staticmethod
    def _sigma(sigma, nrx):
        if sigma is None:
            return None
        sg = np.ascontiguousarray(sigma, dtype=np.float32).reshape(-1)
        if sg.size == 1:
            sg = np.full(nrx, sg[0], dtype=np.float32)
        if sg.size != nrx:
            raise ValueError("sigma: one value, or one per received stream")
        return sg

    def push(self, d_in, in_stride, n, d_out, out_stride, stream=None):
        """transmitted stream t: n samples at d_in + t * in_stride -> received stream r: n samples at d_out + r * out_stride (strides in
        bytes); the samples follow the last call's. Does not synchronise."""
        self._call("pirip_hip_air_push", _dev(d_in), int(in_stride), int(n), _dev(d_out), int(out_stride), _hip_stream(stream))

    def set_sigma(self, sigma, stream=None):
        """new sigma (a number or nrx numbers) for the calls behind this one; does not synchronise"""
        sg = self._sigma(0.0 if sigma is None else sigma, self.nrx)
        self._call("pirip_hip_air_set_sigma", sg.ctypes.data, _hip_stream(stream))

    def reset(self, n0=0, stream=None, age=0):
        """forget the history: the next sample has absolute index n0 and clock age `age`, every earlier one is zero"""
        if age:
            self._call("pirip_hip_air_reset_drift", int(n0), int(age), _hip_stream(stream))
        else:
            self._call("pirip_hip_air_reset", int(n0), _hip_stream(stream))

    def drift(self):
        """(max_slip, how many more samples push() will take): host state, no synchronisation"""
        ms, left = C.c_int32(0), C.c_int64(0)
        self._call("pirip_hip_air_get_drift", C.byref(ms), C.byref(left))
        return ms.value, left.value


class HipSpectrum(_Handle):
    """Band monitor (include/pirip_hip.h section P): averaged power spectra of nstreams wideband IQ streams and the power, peak and peak bin
    of a list of bands, block after block. nfft: 256, 1024 or 4096; hop: nfft (None) or nfft / 2; avg: segments per row; bands: SpecBand
    entries or tuples (stream, lo_hz, hi_hz); in_format: IN_CU8_CSDR or IN_CF32. The incomplete segments and the running row stay on the
    device: any cutting of a stream into push() calls gives the same rows and band entries. db() and occupied() work on what push()
    returned once it is on the host, in numpy and without a device."""
    _c, _Info = "pirip_hip_spec", SpecInfo

    def __init__(self, Fs, nfft, hop=None, avg=1, nstreams=1, bands=(), in_format=IN_CU8_CSDR, device=-1):
        self.bands = [b if isinstance(b, SpecBand) else SpecBand(int(b[0]), int(b[1]), int(b[2])) for b in bands]
        arr = (SpecBand * max(len(self.bands), 1))(*self.bands)
        self._create("pirip_hip_spec_create", int(Fs), int(in_format), int(nfft), int(nfft if hop is None else hop), int(avg), int(nstreams),
                     len(self.bands), C.addressof(arr) if self.bands else None, device)
        self.Fs, self.nfft, self.hop, self.avg, self.nstreams, self.nbands = (self.info.Fs, self.info.nfft, self.info.hop, self.info.avg,
                                                                             self.info.nstreams, self.info.nbands)
        self.scale = float(self.info.scale)
        self.in_format = int(in_format)
        self.bytes_per_sample = 8 if in_format == IN_CF32 else 2

    def window(self):
        return spec_window(self.nfft)

    def band_bins(self, q):
        """(first bin, number of bins) of band q: the bins first, first + 1, ... with wrap-around at nfft"""
        first, count = C.c_int32(0), C.c_int32(0)
        self._call("pirip_hip_spec_band_bins", int(q), C.byref(first), C.byref(count))
        return first.value, count.value

    def nrows(self, n):
        """rows the next push of n samples completes (host arithmetic)"""
        m = int(self._value("pirip_hip_spec_nrows", int(n)))
        if m < 0:
            _chk(m, "pirip_hip_spec_nrows")
        return m

    def push(self, x, rows=None, stream=None):
        """x: a torch tensor on the device, [nstreams, n, 2] uint8 or float32 (or [n, 2] with one stream), the samples that follow the last
        call's. Returns (rows, bands): rows a float32 tensor [nstreams, m, nfft] of the m rows the call completed, unscaled, in FFT bin
        order (None with rows=False), bands a uint8 tensor [nbands, m, 12] of pirip_spec_band_row entries (band_rows() reads it on the
        host). Does not synchronise."""
        import torch
        if x.dim() == 2:
            x = x.unsqueeze(0)
        if x.dim() != 3 or x.shape[0] != self.nstreams or x.shape[2] != 2 or x.element_size() * 2 != self.bytes_per_sample or x.stride(2) != 1 or \
                x.stride(1) != 2:
            raise ValueError("x: [nstreams, n, 2] in the handle's input format, samples contiguous")
        n = int(x.shape[1])
        m = self.nrows(n)
        want_rows = rows is None or bool(rows)
        d_rows = torch.empty((self.nstreams, m, self.nfft), dtype=torch.float32, device=x.device) if want_rows else None
        # (never an empty allocation: a push that completes nothing still hands over a pointer)
        d_bands = torch.empty((self.nbands, max(m, 1), 12), dtype=torch.uint8, device=x.device)
        self.push_raw(x, x.stride(0) * x.element_size(), n, d_rows, self.nfft, max(m, 1) * self.nfft, d_bands if self.nbands else None, max(m, 1),
                      stream)
        return d_rows, d_bands[:, :m]

    def push_raw(self, d_in, in_stride, n, d_rows, row_stride, stream_stride, d_bands, band_stride, stream=None):
        """pirip_hip_spec_push on device pointers or tensors: in_stride in bytes, row_stride / stream_stride in floats, band_stride in entries"""
        self._call("pirip_hip_spec_push", _dev(d_in), int(in_stride), int(n), _dev(d_rows), int(row_stride), int(stream_stride),
                   _dev(d_bands), int(band_stride), _hip_stream(stream))

    def reset(self, stream=None):
        """forget the history: the next sample starts segment 0 of row 0"""
        self._call("pirip_hip_spec_reset", _hip_stream(stream))

    @staticmethod
    def band_rows(bands):
        """push()'s band tensor (or its numpy copy) as a structured array [nbands, m] with the fields power, peak, peak_bin"""
        b = bands.cpu().numpy() if hasattr(bands, "cpu") else np.asarray(bands)
        return np.ascontiguousarray(b).view(SPEC_BAND_ROW_DTYPE).reshape(b.shape[0], b.shape[1])

    def db(self, rows):
        """10 log10(rows scale) of rows [..., nfft] on the host, the bins shifted to dash.py's axis: entry i at -Fs/2 + i Fs/nfft"""
        return spec_db(rows, self.scale)

    def occupied(self, band_rows, noise_band, ratio_db):
        """band_rows: band_rows() of a push, [nbands, m]. True where a band's power per bin exceeds that of band `noise_band` by ratio_db"""
        return spec_occupied(band_rows, [self.band_bins(q)[1] for q in range(self.nbands)], noise_band, ratio_db)


def spec_window(nfft):
    """pirip_hip_spec_window (host only): the nfft floats of the band monitor's window"""
    w = np.zeros(int(nfft), dtype=np.float32)
    _chk(lib().pirip_hip_spec_window(int(nfft), w.ctypes.data), "pirip_hip_spec_window")
    return w


def spec_db(rows, scale):
    """HipSpectrum.db without a handle: rows [..., nfft] (numpy or a tensor), scale = info.scale"""
    r = rows.cpu().numpy() if hasattr(rows, "cpu") else np.asarray(rows)
    with np.errstate(divide="ignore"):
        return np.fft.fftshift(10.0 * np.log10(r.astype(np.float64) * float(scale)), axes=-1)


def spec_occupied(band_rows, nbins, noise_band, ratio_db):
    """HipSpectrum.occupied without a handle: nbins[q] the number of bins of band q"""
    per_bin = band_rows["power"].astype(np.float64) / np.asarray(nbins, dtype=np.float64)[:, None]
    return per_bin > per_bin[int(noise_band)][None, :] * 10.0 ** (float(ratio_db) / 10.0)


def air_fade(f):
    """an AirFade of an AirFade, a tuple (path, doppler_hz, rice_k, key) or a dict: Hz as a float, rounded to whole millihertz"""
    if isinstance(f, AirFade):
        return f
    if isinstance(f, dict):
        f = (f["path"], f["doppler_hz"], f.get("rice_k", 0.0), f.get("key", 0))
    path, hz, k, key = (tuple(f) + (0.0, 0))[:4]
    return AirFade(int(path), int(round(float(hz) * 1000.0)), float(k), int(key))


def air_fade_table(Fs, seed, fade):
    """pirip_hip_air_fade_table (host only): (w int32 [16], theta uint32 [16], scale, los), the integers and floats the kernel reads"""
    f = air_fade(fade)
    w, theta = np.zeros(16, dtype=np.int32), np.zeros(16, dtype=np.uint32)
    scale, los = C.c_float(0), C.c_float(0)
    _chk(lib().pirip_hip_air_fade_table(int(Fs), int(seed), C.byref(f), w.ctypes.data, theta.ctypes.data, C.byref(scale), C.byref(los)),
         "pirip_hip_air_fade_table")
    return w, theta, float(scale.value), float(los.value)


def synth_cu8(Fs, Rs, M, f1_hz, tone_spacing, d_bits, bits_stride, nsym, d_out, out_stride, nsamp,
              amp=32.0, sigma=0.0, seed=1, skip=None, stream=0):
    """Device-side fsk_mod -c | u8 quantiser [| AWGN] for len(f1_hz) streams (include/pirip_hip.h B2).
    d_bits / d_out are device pointers; f1_hz / skip are host integer sequences."""
    f1 = np.ascontiguousarray(f1_hz, dtype=np.int32)
    sk = None if skip is None else np.ascontiguousarray(skip, dtype=np.int32)
    assert sk is None or sk.size == f1.size
    _chk(lib().pirip_hip_synth_cu8(Fs, Rs, M, int(f1.size), f1.ctypes.data, tone_spacing,
                                   None if sk is None else sk.ctypes.data, d_bits, bits_stride, nsym,
                                   d_out, out_stride, nsamp, amp, sigma, seed, stream), "pirip_hip_synth_cu8")


class HipLdpc(_Handle):
    """nstreams FSK_LDPC receivers (include/pirip_hip.h section E): soft decisions -> status / payload records."""
    _c, _Info = "pirip_hip_ldpc", LdpcInfo

    def __init__(self, code_path, M, Nsym=50, nstreams=1, device=-1):
        self._create("pirip_hip_ldpc_create", code_path.encode(), M, Nsym, nstreams, device)
        self.M, self.Nsym, self.nstreams = M, Nsym, nstreams
        self.n, self.k, self.Nbits, self.data_bytes = self.info.n, self.info.k, self.info.nbits_per_call, self.info.data_bytes

    def reset(self, stream=0):
        self._call("pirip_hip_ldpc_reset", stream)

    def llr_history(self, s=0):
        """The 2 * bits_per_frame binary16 soft bits receiver s carries into its next call, oldest first (pirip_hip_ldpc_get_llr_history)."""
        out = np.zeros(2 * self.info.bits_per_frame, dtype=np.float16)
        self._call("pirip_hip_ldpc_get_llr_history", s, out.ctypes.data)
        return out

    def layout_conflicts(self):
        """(identity layout's, layout in use's) bank conflicts per decoder iteration (pirip_hip_ldpc_get_layout_conflicts)."""
        ident, used = C.c_int(0), C.c_int(0)
        self._call("pirip_hip_ldpc_get_layout_conflicts", C.byref(ident), C.byref(used))
        return ident.value, used.value

    def rx_batch(self, d_rx_filt, filt_stride, d_ncalls, ncalls, d_status, d_payload, d_info, stream=0):
        self._call("pirip_hip_ldpc_rx_batch", d_rx_filt, filt_stride, d_ncalls, ncalls, d_status, d_payload, d_info, stream)

    def chain_batch(self, dem, d_in, in_stride, nsamp, d_status, d_payload, d_info, d_nframes, d_consumed, max_frames,
                    d_stats=0, stats_stride=0, stream=0):
        """pirip_hip_fsk_ldpc_rx_batch: IQ of every stream of HipDemod `dem` -> records of this receiver's streams (device pointers)."""
        name = "pirip_hip_fsk_ldpc_rx_batch"
        _chk(self.L.pirip_hip_fsk_ldpc_rx_batch(dem._ptr(name), self._ptr(name), d_in, in_stride, nsamp, d_status, d_payload, d_info, d_stats,
                                                stats_stride, d_nframes, d_consumed, max_frames, stream), name)

    @staticmethod
    def chain_batch_groups(groups, in_stride, nsamp, max_frames, stats_stride=0, stream=0):
        """pirip_hip_fsk_ldpc_rx_batch_groups: groups = [(HipLdpc, HipDemod, d_in, d_status, d_payload, d_info, d_nframes, d_consumed[, d_stats]), ...]"""
        name = "pirip_hip_fsk_ldpc_rx_batch_groups"
        arr = (ChainGroup * len(groups))()
        for i, g in enumerate(groups):
            ld, dem, d_in, d_status, d_payload, d_info, d_nframes, d_consumed = g[:8]
            arr[i] = ChainGroup(dem._ptr(name), ld._ptr(name), d_in, d_status, d_payload, d_info, g[8] if len(g) > 8 else None, d_nframes,
                                d_consumed)
        _chk(lib().pirip_hip_fsk_ldpc_rx_batch_groups(arr, len(groups), in_stride, nsamp, stats_stride, max_frames, stream), name)

    def last_path_fused(self):
        return self._value("pirip_hip_fsk_ldpc_last_path") == 1

    def rx_host(self, rx_filt_calls):
        r = np.ascontiguousarray(rx_filt_calls, dtype=np.float32).reshape(-1, self.M * self.Nsym)
        n = r.shape[0]
        status = np.zeros(n, dtype=np.uint8)
        payload = np.zeros((n, self.data_bytes), dtype=np.uint8)
        info = np.zeros((n, LDPC_INFO_PER_CALL), dtype=np.int32)
        self._call("pirip_hip_ldpc_rx_host", r.ctypes.data, n, status.ctypes.data, payload.ctypes.data, info.ctypes.data)
        return status, payload, info


class HipRx(_Handle):
    """Streaming receiver over live channels (include/pirip_hip.h section G): one block per channel per call, each channel's unconsumed
    tail carried on the device. dem: HipDemod; ldpc: HipLdpc or None (records out instead of bits); dec: HipDecim or None (u8 IQ at
    the tuner rate in instead of modem-rate samples); chan: HipChan or None (wideband u8 IQ captures in, one row per capture, each
    channel of the channelizer a channel of dem; exclusive with dec); block: input samples per channel (per capture with chan) per call.
    The handles must outlive the receiver."""
    _c = "pirip_hip_rx"

    def __init__(self, dem, ldpc=None, dec=None, block=None, chan=None):
        if dec is not None and chan is not None:
            raise ValueError("HipRx: dec and chan are mutually exclusive")
        self.dem, self.ldpc, self.dec, self.chan = dem, ldpc, dec, chan
        name = "pirip_hip_rx_create_chan" if chan is not None else "pirip_hip_rx_create"
        self._create(name, dem._ptr(name), _ptr_of(ldpc, name), _ptr_of(chan if chan is not None else dec, name), int(block))
        self.block, self.nstreams = int(block), dem.nstreams
        self.ninputs = chan.ninputs if chan is not None else dem.nstreams
        self.max_frames = int(self._value("pirip_hip_rx_max_frames"))

    def input(self):
        """(device pointer of channel 0's next block, stride in bytes): the zero-copy landing zone (pirip_hip_rx_input)."""
        p, st = C.c_void_p(), C.c_size_t(0)
        self._call("pirip_hip_rx_input", C.byref(p), C.byref(st))
        return int(p.value), int(st.value)

    def process(self, d_bits=0, bits_stride=0, d_filt=0, filt_stride=0, d_status=0, d_payload=0, d_info=0, d_stats=0, stats_stride=0,
                d_nframes=0, stream=0):
        """Raw device pointers (ints); enqueues on `stream`, does not synchronise."""
        self._call("pirip_hip_rx_process", d_bits, bits_stride, d_filt, filt_stride, d_status, d_payload, d_info, d_stats,
                   stats_stride, d_nframes, stream)

    def push(self, d_in, in_stride, d_bits=0, bits_stride=0, d_filt=0, filt_stride=0, d_status=0, d_payload=0, d_info=0, d_stats=0,
             stats_stride=0, d_nframes=0, stream=0):
        """process() after copying channel s's block from d_in + s * in_stride (device) into the input."""
        self._call("pirip_hip_rx_push", d_in, in_stride, d_bits, bits_stride, d_filt, filt_stride, d_status, d_payload, d_info,
                   d_stats, stats_stride, d_nframes, stream)

    def counters(self):
        """(consumed_total int64[nstreams], backlog int32[nstreams]) -- synchronises."""
        tot = np.zeros(self.nstreams, dtype=np.int64)
        bl = np.zeros(self.nstreams, dtype=np.int32)
        self._call("pirip_hip_rx_get_counters", tot.ctypes.data, bl.ctypes.data)
        return tot, bl

    def reset(self, stream=0):
        self._call("pirip_hip_rx_reset", stream)
