"""include/pirip_hip.h section G (streaming receiver) without a GPU: the built library exports the new entry points, and the header
declares them so that a plain-C caller compiles and links against libpirip_hip.so (tests/cprog/stream_rx_like_multichannel.c)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RX_SYMBOLS = ("pirip_hip_rx_create", "pirip_hip_rx_destroy", "pirip_hip_rx_max_frames", "pirip_hip_rx_input", "pirip_hip_rx_process",
              "pirip_hip_rx_push", "pirip_hip_rx_get_counters", "pirip_hip_rx_reset")


def test_library_exports_the_streaming_receiver(built_lib):
    import pirip_amd
    out = subprocess.run(["nm", "-D", "--defined-only", pirip_amd.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    for n in RX_SYMBOLS:
        assert n in exported, n
        assert hasattr(built_lib, n), n


def test_header_compiles_as_plain_c_and_links(built_lib, tmp_path):
    import pirip_amd
    libdir = os.path.dirname(pirip_amd.lib_path())
    exe = str(tmp_path / "stream_rx_like_multichannel")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cprog", "stream_rx_like_multichannel.c"), "-L", libdir, "-lpirip_hip",
                           "-Wl,-rpath," + libdir, "-lm"])
    assert os.path.exists(exe)
