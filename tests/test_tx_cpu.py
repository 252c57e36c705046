"""FSK_LDPC transmit (include/pirip_hip.h section I), what can be checked without a device: the interface exists, the CLI refuses what
the framer refuses and fails loudly without a GPU, and the float64 restatement of the modulator's phase formula (tests/txref.py, the
checker of tests/test_tx.py) describes the signal codec2's float recursion sends."""
import ctypes as C
import os
import subprocess

import numpy as np

import sigutil
import txref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "pirip_amd", "bin")
CODE = os.path.join(ROOT, "pirip_amd", "data", "standin_256_512_4.code")
SYMBOLS = ["pirip_hip_tx_create", "pirip_hip_tx_destroy", "pirip_hip_tx_get_info", "pirip_hip_tx_set_tones", "pirip_hip_tx_set_gaps",
           "pirip_hip_tx_reset", "pirip_hip_tx_max_syms", "pirip_hip_tx_frame", "pirip_hip_tx_modulate", "pirip_hip_tx_records_to_iq"]


def _non_accumulator(tmp_path):
    """the stand-in code with one sub-diagonal parity entry removed: still a valid code file, no linear-time encoder"""
    lines = open(CODE).read().split("\n")
    i = next(k for k, ln in enumerate(lines) if ln.startswith("rows"))
    k = int(next(ln for ln in lines if ln.startswith("k ")).split()[1])
    row = lines[i + 1 + 5].split()
    assert str(k + 4) in row and str(k + 5) in row
    row.remove(str(k + 4))
    lines[i + 1 + 5] = " ".join(row)
    out = os.path.join(str(tmp_path), "broken.code")
    with open(out, "w") as f:
        f.write("\n".join(lines))
    return out


def test_header_declares_section_i_and_the_library_exports_it(built_lib):
    import pirip_amd
    hdr = open(os.path.join(ROOT, "include", "pirip_hip.h")).read()
    assert "section I : FSK_LDPC transmit" in hdr
    for name in SYMBOLS:
        assert name + "(" in hdr, name
        assert hasattr(built_lib, name), name
    assert hasattr(pirip_amd, "HipTx")
    # section I only adds symbols: the ABI numbers stand
    abi, spf, sz = C.c_int(0), C.c_int(0), C.c_size_t(0)
    built_lib.pirip_hip_abi(C.byref(abi), C.byref(spf), C.byref(sz))
    assert abi.value == 2 and spf.value == 10
    # argument checks come before the device is looked for
    h = C.c_void_p()
    assert built_lib.pirip_hip_tx_create(CODE.encode(), 240000, 7000, 2, 1, -1, C.byref(h)) == -2      # Fs % Rs
    assert built_lib.pirip_hip_tx_create(CODE.encode(), 240000, 10000, 3, 1, -1, C.byref(h)) == -2     # M
    assert built_lib.pirip_hip_tx_create(CODE.encode(), 1 << 25, 1 << 10, 2, 1, -1, C.byref(h)) == -6  # Fs > 2^24
    assert built_lib.pirip_hip_tx_create(b"/nonexistent.code", 240000, 10000, 2, 1, -1, C.byref(h)) == -1


def test_tx_create_refuses_a_code_without_the_accumulator_shape(built_lib, tmp_path):
    h = C.c_void_p()
    assert built_lib.pirip_hip_tx_create(_non_accumulator(tmp_path).encode(), 240000, 10000, 2, 1, -1, C.byref(h)) == -2
    assert not h.value


def test_fsk_ldpc_tx_cli_exit_codes(built_lib, tmp_path):
    exe = os.path.join(BIN, "fsk_ldpc_tx")
    framer = os.path.join(BIN, "fsk_ldpc_framer")
    modem = ["240000", "10000", "10000", "10000"]

    def run(args):
        return subprocess.run([exe] + args, input=b"", capture_output=True)

    def run_framer(args):
        return subprocess.run([framer] + args, input=b"", capture_output=True)

    # the framer's refusals, with the framer's exit codes
    broken = _non_accumulator(tmp_path)
    for tx_args, fr_args in (
            (["--testframes", "1"] + modem + ["/dev/zero", "-"], ["--testframes", "1", "/dev/zero", "-"]),                      # no --code
            (["--code", CODE, "-m", "3"] + modem + ["-", "-"], ["--code", CODE, "-m", "3", "-", "-"]),                            # M
            (["--code", "/nonexistent.code"] + modem + ["-", "-"], ["--code", "/nonexistent.code", "-", "-"]),                    # code file
            (["--code", broken, "--testframes", "1"] + modem + ["/dev/zero", "-"], ["--code", broken, "--testframes", "1", "/dev/zero", "-"])):
        a, b = run(tx_args), run_framer(fr_args)
        assert a.returncode == b.returncode and a.returncode in (1, 2), (tx_args, a.returncode, b.returncode, a.stderr)
        assert a.stdout == b""
    assert run(["--code", broken, "--testframes", "1"] + modem + ["/dev/zero", "-"]).returncode == 2
    # its own arguments
    assert run(["--code", CODE, "240000", "7000", "10000", "10000", "-", "-"]).returncode == 1          # Fs % Rs
    assert run(["--code", CODE, "--format", "s16"] + modem + ["-", "-"]).returncode == 1
    assert run(["--code", CODE, "-m", "4", "--gap", "3"] + modem + ["-", "-"]).returncode == 1            # half a symbol
    assert run(["--code", CODE, "240000", "10000", "-", "-"]).returncode == 1                            # missing modem arguments
    import pirip_amd
    if pirip_amd.device_count() == 0:
        # no device: loud, non-zero, and not one byte of output
        p = run(["--code", CODE, "--testframes", "2"] + modem + ["/dev/zero", "-"])
        assert p.returncode == 3 and p.stdout == b"" and b"no usable HIP device" in p.stderr


def test_phase_formula_is_what_the_float_recursion_sends(oracle, built_lib):
    """One burst (preamble + 3 frames) through the CPU modulator (fsk_mod's float recursion, oracle mod_c) and through the exact-phase
    formula in float64: the two differ only by the recursion's drift, far below half a u8 level at amp = 32 -- the phase convention
    (advance before output, MSB-first symbols, tones f1 + m * shift) is the modulator's."""
    for M, cfg in ((2, dict(sigutil.CFG1, P=8)), (4, sigutil.CFG4)):
        p = subprocess.run([os.path.join(BIN, "fsk_ldpc_framer"), "--code", CODE, "-m", str(M), "--testframes", "3", "--seq", "/dev/zero", "-"],
                           capture_output=True)
        assert p.returncode == 0
        bits = np.frombuffer(p.stdout, dtype=np.uint8)
        bits = bits[:bits.size - bits.size % (50 * (1 if M == 2 else 2))]       # the fsk_mod tool sends whole blocks of 50 symbols
        x = sigutil.mod_complex(oracle, cfg, bits).astype(np.float64)
        Ts = cfg["Fs"] // cfg["Rs"]
        y = txref.mod_f64(txref.bits_to_syms(bits, M), cfg["f1"], cfg["shift"], cfg["Fs"], Ts)
        assert x.shape[0] == y.size
        d = max(float(np.max(np.abs(x[:, 0] - y.real))), float(np.max(np.abs(x[:, 1] - y.imag))))
        print(f"M={M}: {y.size} samples, largest component difference to the float recursion {d:.3e}")
        assert d < 0.5 / 32.0


def test_float64_formula_meets_few_rounding_ties_on_the_test_tones():
    """tests/test_tx.py allows one u8 level of difference only where the float64 value is within BOUND * amp of a tie, and caps the share
    of such samples at 1e-3: the restatement alone must stay under that cap for the tones used there."""
    import test_tx
    rng = np.random.default_rng(3)
    assert 5e-7 < txref.BOUND < 2e-6
    for (Fs, Rs, M, f1s, shift) in test_tx.MOD_SHAPES:
        Ts = Fs // Rs
        for f1 in f1s:
            syms = rng.integers(0, M, 2000).astype(np.uint8)
            _, v = txref.quantise(txref.mod_f64(syms, f1, shift, Fs, Ts), 32.0)
            share = float(np.mean(txref.near_tie(v, 32.0)))
            assert share < 1e-3 / 4, (Fs, Rs, M, f1, share)
