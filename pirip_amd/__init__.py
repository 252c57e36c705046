"""pirip_amd -- MI355X-native FSK receive path (IQ -> bits) behind pirip's tool/library boundary.

The product is the C-ABI shared library ``pirip_amd/lib/libpirip_hip.so`` (include/pirip_hip.h)
and the CLI tools under ``pirip_amd/bin``. This package is the thin Python binding used by
bench.py and the tests; it never imports the CPU oracle and has no CPU compute path.
"""
from .binding import (  # noqa: F401
    PiripError, FskParams, HipDemod, HipDecim, lib, lib_path, build, device_count, selftest_sqrt, selftest_div,
    StreamState, kernel_source_hash, selftest_atan2,
    IN_CU8_FSKDEMOD, IN_CU8_CSDR, IN_CS16, IN_CF32, STATS_PER_FRAME,
    HipTestBits, testframe_payload, HipRepeater, HipPing, PingConfig, PingEntry, PING_ENTRY_DTYPE, HipAir, AirPath, AirPathEx, AirInfo,
    AirFade, air_fade, air_fade_table, launch_first_tail_block,
    HipSpectrum, SpecBand, SpecInfo, SPEC_BAND_ROW_DTYPE, spec_window, spec_db, spec_occupied,
    DivConfig, DivEntry, DivInfo, DIV_ENTRY_DTYPE,
    PktConfig, PktEntry, PktInfo, PKT_ENTRY_DTYPE, PktFecConfig, PktFecInfo, ArqConfig, ArqEntry, ArqInfo, ARQ_ENTRY_DTYPE,
    MacConfig, MacInfo, MAC_IDLE, MAC_CONTEND, MAC_HOLD,
    HipLdpc, HipRx, HipChan, HipTx, HipMux, HipTxStream, MUX_FIR, MUX_LINEAR, TX_CARRIER_OFF, STANDIN_CODE, RX_TRIAL_SYNC, RX_SYNC, RX_BITS, RX_BIT_ERRORS, LDPC_INFO_PER_CALL,
)
from .diversity import HipDiversity  # noqa: F401
from .packet import HipPacket, HipPacketFec  # noqa: F401
from .arq import HipArq  # noqa: F401
from .mac import HipMac  # noqa: F401
