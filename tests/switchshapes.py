"""The library's opt-in environment switches: which test launches each of them, the decimator's launch rules restated, and the shapes the
switch tests run. Pure Python, no GPU: tests/test_switches_cpu.py holds the table to the sources and the rows to the restated rules, and
proves on the oracle alone that each arithmetic row can tell its arithmetics apart; tests/test_switches.py runs the rows on the device.

SWITCHES has one entry per PIRIP_* name that a getenv() under pirip_amd/csrc or pirip_amd/tools reads:
    ("test", "tests/<file>.py::<test>")   a test that sets the switch and launches what it selects (the file names the switch)
    ("exempt", reason)                    no launch test applies
A switch added to the sources fails the CPU suite until it has a launch test or a reason why none applies."""
from collections import namedtuple

SW = "tests/test_switches.py::"
SWITCHES = {
    # ---- launched by tests/test_switches.py
    "PIRIP_FFT_FMA": ("test", SW + "test_fused_fft_multiply_equals_the_fused_oracle"),
    "PIRIP_DECIM_FMA": ("test", SW + "test_decimator_opt_in_arithmetics_are_their_formulas_bit_for_bit"),
    "PIRIP_DECIM_LUT": ("test", SW + "test_decimator_table_conversion_is_the_exact_oracle"),
    "PIRIP_DECIM_TPW": ("test", SW + "test_decimator_multi_tile_walk"),
    "PIRIP_GENERAL_THREADS": ("test", SW + "test_general_kernel_thread_counts_equal_the_oracle"),
    "PIRIP_LAYOUT_TRIES": ("test", SW + "test_ldpc_storage_layouts_decode_the_same_words"),
    "PIRIP_BLOCK_STAGGER": ("test", SW + "test_block_stagger_changes_no_output_word"),
    "PIRIP_CAPTURE_REPLICAS": ("test", SW + "test_capture_replicas_and_pinned_frames_change_no_output_word"),
    "PIRIP_CAPTURE_PIN_FRAMES": ("test", SW + "test_capture_replicas_and_pinned_frames_change_no_output_word"),
    "PIRIP_EST_BAND": ("test", SW + "test_env_forms_equal_the_api_forms"),
    "PIRIP_EXACT0": ("test", SW + "test_env_forms_equal_the_api_forms"),
    "PIRIP_CSDR_BLOCKS": ("test", SW + "test_csdr_tool_block_count_changes_no_output_byte"),
    "PIRIP_FSK_DEMOD_FRAMES": ("test", SW + "test_fsk_demod_tool_call_sizes_change_no_output_byte"),
    "PIRIP_FSK_DEMOD_SLOTS": ("test", SW + "test_fsk_demod_tool_call_sizes_change_no_output_byte"),
    # ---- launched by tests that were there before
    "PIRIP_DECIM_SHARED": ("test", "tests/test_gpu_parity.py::test_convert_once_decimator_equals_the_per_output_one"),
    "PIRIP_CAPTURE_SEG_FRAMES": ("test", "tests/test_capture.py::test_capture_equals_the_sequential_read_loop"),
    "PIRIP_CAPTURE_SEQUENTIAL": ("test", "tests/test_capture.py::test_capture_equals_the_sequential_read_loop"),
    "PIRIP_CHAIN_OVERLAP_DECODER": ("test", "tests/test_ldpc.py::test_chain_split_into_two_stream_ranges_writes_the_same_records"),
    "PIRIP_CHAIN_SPLIT_EIGHTHS": ("test", "tests/test_ldpc.py::test_chain_split_into_two_stream_ranges_writes_the_same_records"),
    "PIRIP_CHAIN_SPLIT_MIN": ("test", "tests/test_ldpc.py::test_chain_split_into_two_stream_ranges_writes_the_same_records"),
    "PIRIP_CHAIN_TEST_FAIL": ("test", "tests/test_ldpc.py::test_chain_split_joins_the_callers_stream_when_a_range_fails"),
    "PIRIP_CODE_DIR": ("test", "tests/test_rtl_fsk_cli.py::test_reference_rtl_fsk_command_line_verbatim"),
    "PIRIP_FORCE_GENERAL": ("test", "tests/test_gpu_parity.py::test_general_kernel_odd_stream_counts_share_tables"),
    "PIRIP_FRAME_CACHE": ("test", "tests/test_wave_frame_cache.py::test_steady_moving_tones_and_nin_steps_hit_and_miss_alike"),
    "PIRIP_FSK_DEMOD_REPORT": ("test", "tests/test_capture.py::test_fsk_demod_on_a_file_uses_the_capture_route_and_matches_the_pipe"),
    "PIRIP_IQ_FILE": ("test", "tests/test_rtl_fsk_cli.py::test_reference_rtl_fsk_command_line_verbatim"),
    "PIRIP_KERNEL": ("test", "tests/test_gpu_parity.py::test_exact_kernel_equals_the_oracle_bit_for_bit_under_noise"),
    "PIRIP_LDPC_DECODER": ("test", "tests/test_ldpc_decoders.py::test_decoder_shape_matrix"),
    "PIRIP_LDPC_GENERIC": ("test", "tests/test_ldpc_decoders.py::test_decoder_shape_matrix"),
    "PIRIP_RCCL_SESSION": ("test", "tests/test_gather_fake_nccl.py::test_cpp_gather_slots_layout_and_rendezvous"),
    "PIRIP_RCCL_TIMEOUT_S": ("test", "tests/test_gather_fake_nccl.py::test_rendezvous_times_out_with_a_message_when_rank0_never_comes"),
    "PIRIP_RECALLED": ("test", "tests/test_oracle.py::test_pin_day_drill_names_the_recalled_constant_that_differs"),
    "PIRIP_RTL_FSK_BANNER": ("test", "tests/test_rtl_fsk_cli.py::test_reference_rtl_fsk_command_line_verbatim"),
    "PIRIP_RTL_FSK_RULES": ("test", "tests/test_rtl_fsk_cli.py::test_rtl_fsk_recalled_rules_are_data"),
    "PIRIP_SHIM_EYE": ("test", "tests/test_gpu_parity.py::test_library_boundary_c_program_written_like_upstream"),
    # ---- nothing to launch
    "PIRIP_WAVE_STOP": ("exempt", "read behind #ifdef PIRIP_WAVE_TIMING, which no build of the library defines"),
    "PIRIP_CAPTURE_DEBUG": ("exempt", "only prints the capture's pass log to stderr"),
}


# ---- the decimator's launch rules (pirip_amd/csrc/decim_kernels.hip), restated -------------------------------------------------------------
SHARED_D, SYSTOLIC_D = (45, 50), (6, 9, 10, 18, 30)       # shapes with a decim_shared_kernel / decim_systolic_kernel instance (79 taps)
FILL_WGS = 8 * 256 * 6                                    # the walk is halved while the grid has fewer workgroups than this


def filter_len(transition_bw):
    """csdr's firdes_filter_len on a float32 argument"""
    import numpy as np
    n = int(4.0 / float(np.float32(transition_bw)))
    return n + 1 if n % 2 == 0 else n


def decim_plan(D, transition_bw=0.05, lut=False, shared_env=True):
    """pirip_hip_decim_create: taps, padded taps, the general kernel's tile, which convert-once kernel exists and its tile.
    lut: PIRIP_DECIM_LUT is set; shared_env False: PIRIP_DECIM_SHARED=0."""
    L = filter_len(transition_bw)
    tile = 256
    while tile > 1 and 2 * ((tile - 1) * D + L) + 32 > 48 * 1024:
        tile //= 2
    arith = not lut
    on = shared_env and arith and L == 79
    shared = 1 if on and D in SHARED_D else 2 if on and D in SYSTOLIC_D else 0
    tile_sh = 4 * (64 - ((L + D - 1) // D - 1)) if shared == 2 else 4 * 63
    return dict(D=D, L=L, Lp=(L + 3) & ~3, tile=tile, arith=arith, shared=shared, tile_sh=tile_sh)


def decim_launch(plan, n_in, nstreams, mode=0, aligned=True, env_tpw=None):
    """pirip_hip_decim_batch: outputs, kernel, tile, tiles, tiles per workgroup, workgroups per stream.
    mode: the tap-loop arithmetic in force (0 where the plan has no arithmetic conversion); aligned: base address and stride both even."""
    D, Lp = plan["D"], plan["Lp"]
    n_out = 0 if n_in < Lp else (n_in - Lp) // D + 1
    sh = bool(plan["shared"]) and mode == 0 and aligned
    tile = plan["tile_sh"] if sh else plan["tile"]
    ntiles = (n_out + tile - 1) // tile
    tpw = env_tpw if env_tpw and env_tpw > 0 else 8
    while tpw > 1 and ((ntiles + tpw - 1) // tpw) * nstreams < FILL_WGS:
        tpw //= 2
    kernel = "systolic" if sh and plan["shared"] == 2 else "shared" if sh else "general"
    # the general kernel's loop per output: the table loop unless the conversion is arithmetic and the staged window starts on an even byte
    loop = "n/a" if sh else "taps" if plan["arith"] and aligned else "table"
    return dict(n_out=n_out, kernel=kernel, tile=tile, ntiles=ntiles, tpw=tpw, nwg=(ntiles + tpw - 1) // tpw, loop=loop)


# ---- rows --------------------------------------------------------------------------------------------------------------------------------
# opt-in arithmetics: (D, transition_bw, the kernel mode 0 takes at an aligned address)
ARITH_ROWS = [(45, 0.05, "shared"), (6, 0.05, "systolic"), (7, 0.0975, "general")]
ARITH_STREAMS = 3
# PIRIP_DECIM_LUT: (D, the general kernel's tile)
LUT_ROWS = [(45, 256), (6, 256), (200, 64)]


def arith_n_in(D):
    """two full tiles of either kernel and a partial one"""
    return D * 600 + 91


# The bytes of the arithmetic rows: three streams from byte ARITH_OFF of one buffer, once at an even stride (every stream 2-byte aligned)
# and once at an odd one (the middle stream starts on an odd address). Seeded by D, except where that draw leaves no s16 output of the
# aligned streams on which exact and fma differ (truncation to s16 keeps about one such difference in a thousand words):
# test_switches_cpu.py asserts that both output types of every row tell all three modes apart.
ARITH_OFF = 2
ARITH_SEEDS = {6: 100, 7: 100}


def arith_strides(D):
    return {"aligned": 2 * arith_n_in(D) + 6, "odd stride": 2 * arith_n_in(D) + 7}


def arith_host(D):
    return random_bytes(ARITH_SEEDS.get(D, D), ARITH_OFF + ARITH_STREAMS * max(arith_strides(D).values()) + 64)


def arith_stream(host, D, layout, s):
    """stream s of a layout as u8 IQ [n_in, 2]"""
    import numpy as np
    n_in, o = arith_n_in(D), ARITH_OFF + s * arith_strides(D)[layout]
    return np.ascontiguousarray(host[o:o + 2 * n_in]).reshape(n_in, 2)


# the multi-tile walk. kernel / tile / tpw / last: what the row claims (last = tiles the last workgroup of a stream walks);
# partial: outputs of the last tile; pad: bytes between streams (even); base: byte offset of the first stream (even)
Walk = namedtuple("Walk", "name D nstreams ntiles kernel tile tpw last partial pad base")
WALK_ROWS = [
    Walk("general_tpw2", 7, 6144, 3, "general", 256, 2, 1, 9, 6, 0),
    Walk("systolic_tpw2", 6, 6144, 3, "systolic", 204, 2, 1, 60, 2, 2),
    Walk("shared_tpw2", 45, 6144, 3, "shared", 252, 2, 1, 70, 10, 0),
    Walk("general_tpw8", 2, 1536, 65, "general", 256, 8, 1, 5, 4, 0),
    # With three tiles and a walk of two, a workgroup that started its walk at tile blockIdx.x instead of blockIdx.x * tpw would still
    # cover every tile (0-1 and 1-2). Five tiles leave tile 4 to the third workgroup alone: the two convert-once kernels again, where a
    # wrong first tile shows (the general kernel has the 65-tile row for that).
    Walk("systolic_tpw2_5tiles", 6, 4096, 5, "systolic", 204, 2, 1, 9, 2, 0),
    Walk("shared_tpw2_5tiles", 45, 4096, 5, "shared", 252, 2, 1, 9, 6, 2),
]
WALK_BY_NAME = {r.name: r for r in WALK_ROWS}
ORACLE_ALL_STREAMS_BELOW = 6e8       # multiply-adds per component the scalar oracle does in about a second


def walk_n_in(r, plan):
    n_out = (r.ntiles - 1) * r.tile + r.partial
    return (n_out - 1) * r.D + plan["Lp"] + r.D // 2


def walk_oracle_streams(r, plan):
    """streams held to the oracle: all where that is about a second of scalar work, else every 64th, the first and the last"""
    n_out = (r.ntiles - 1) * r.tile + r.partial
    if r.nstreams * n_out * plan["Lp"] <= ORACLE_ALL_STREAMS_BELOW:
        return list(range(r.nstreams))
    return sorted(set(range(0, r.nstreams, 64)) | {0, r.nstreams - 1})


def random_bytes(seed, n):
    import numpy as np
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


# ---- the fused FFT multiply (PIRIP_FFT_FMA=1): inputs and the oracle's replay ----------------------------------------------------------------
FFT_INPUTS = ("clean", "awgn9", "ppm400")
FFT_BATCH = ("clean", "awgn9", "ppm400", "clean13", "awgn9b")     # five streams: a partial workgroup at four streams per workgroup
_cache = {}


def fft_input(ob, sigutil, name):
    """u8 IQ of the headline shape (sigutil.CFG1, fsk_demod -d): clean test bits from a start offset, random bits at Eb/N0 = 9 dB, and a
    sample clock 400 ppm fast that moves nin. Computed once, read-only."""
    if name not in _cache:
        c = sigutil.CFG1
        if name in ("clean", "clean13"):
            u8 = sigutil.make_u8_stream(ob, c, 12000, offset=7 if name == "clean" else 13)[0]
        elif name in ("awgn9", "awgn9b"):
            u8 = sigutil.make_u8_stream(ob, c, 12000, seed=3 if name == "awgn9" else 4, ebno_db=9.0, random_bits=True, amp=18.0)[0]
        else:
            import numpy as np
            x = sigutil.mod_complex(ob, c, ob.get_test_bits(12000))
            n, ppm = x.shape[0], 400e-6
            t = np.arange(int(n / (1 + ppm) - 2)) * (1 + ppm)
            i0 = np.floor(t).astype(int)
            fr = (t - i0)[:, None].astype(np.float32)
            u8 = np.ascontiguousarray(ob.quantise_cu8((1 - fr) * x[i0] + fr * x[np.minimum(i0 + 1, n - 1)]))
        u8.setflags(write=False)
        _cache[name] = u8
    return _cache[name]


def oracle_fft_run(ob, sigutil, u8, fused, first_frame_unfused=False, cfg=None):
    """The oracle on u8 with the estimator FFT's multiply unfused or fused; first_frame_unfused: the switch is flipped after frame 0 (the
    product's exact first-frame prologue runs in the general kernel's unfused body). Returns (result, Sf); the switch is left off."""
    import numpy as np
    from parity import oracle_Sf
    c = cfg or sigutil.CFG1
    o = ob.OracleFsk(c["Fs"], c["Rs"], c["M"], P=c["P"], est_min=c["est_min"], est_max=c["est_max"])
    try:
        if fused and first_frame_unfused:
            n0 = o.nin()
            r0 = o.demod(u8[:n0], ob.IN_CU8_FSKDEMOD)
            assert r0["nframes"] == 1 and r0["consumed"] == n0
            ob.set_fft_fused(True)
            r1 = o.demod(u8[n0:], ob.IN_CU8_FSKDEMOD)
            r = {k: np.concatenate([r0[k], r1[k]]) for k in ("bits", "rx_filt", "stats", "timing_cond")}
            r["nframes"], r["consumed"] = 1 + r1["nframes"], n0 + r1["consumed"]
        else:
            ob.set_fft_fused(fused)
            r = o.demod(u8, ob.IN_CU8_FSKDEMOD)
    finally:
        ob.set_fft_fused(False)
    ndft = 1 << (int(c["Fs"] / (0.1 * c["Rs"])) - 1).bit_length()
    Sf = oracle_Sf(ob, o, ndft)
    return r, Sf
