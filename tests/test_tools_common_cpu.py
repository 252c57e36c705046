"""pirip_amd/tools/tool_common.hpp and tx_records.hpp -- the host code the command-line tools share -- checked by a stand-alone
program (tests/cprog/tool_common_check.cpp) under the address and undefined-behaviour sanitizers: no HIP, no libpirip_hip.so."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shared_tool_code_under_sanitizers(tmp_path):
    (tmp_path / "bin").mkdir()                      # resolve_code's third place is <exe dir>/../data: inside tmp_path
    (tmp_path / "work").mkdir()
    exe = str(tmp_path / "bin" / "tool_common_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",     # the runtimes linked in: the program starts under any preloaded library
                           "-I", os.path.join(ROOT, "pirip_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "cprog", "tool_common_check.cpp"), os.path.join(ROOT, "pirip_amd", "csrc", "fsk_ldpc.cpp")])
    # only the pure-host parts are used: nothing of the library or of the HIP runtime is linked
    needed = subprocess.run(["ldd", exe], capture_output=True, text=True, check=True).stdout
    assert "pirip_hip" not in needed and "amdhip" not in needed, needed
    env = {k: v for k, v in os.environ.items() if k != "PIRIP_CODE_DIR"}
    p = subprocess.run([exe, str(tmp_path / "work")], capture_output=True, text=True, env=env)
    assert p.returncode == 0 and p.stdout == "ok\n", p.stderr
