"""The host rule of the wave kernel's launch tail (fsk_plan.cpp: launch_first_tail_block, launch_resident_blocks) as a pure function
through the C-ABI, pirip_hip_launch_first_tail_block -- no device. R = streams per CU / streams per workgroup x compute units workgroups
are resident at once; a launch of nblocks > R workgroups raises the last R of them, a smaller one none (first raised block = nblocks).
(One level only: the variant with three levels over the thirds of the window measured the same and was not kept)"""
import pytest

import pirip_amd

SHAPES = [(12, 4, 256), (12, 4, 1), (8, 2, 256), (16, 4, 304), (8, 4, 7), (12, 4, 5)]     # (streams per CU, streams per workgroup, CUs)


@pytest.mark.parametrize("spc,wpb,cus", SHAPES)
def test_first_tail_block(built_lib, spc, wpb, cus):
    R = spc // wpb * cus
    for nblocks in (0, 1, R - 1, R, R + 1, R + 2, 2 * R - 1, 2 * R, 2 * R + 1, 5 * R + R // 3, 1 << 20):
        first = pirip_amd.launch_first_tail_block(nblocks, spc, wpb, cus)
        assert first == (nblocks - R if nblocks > R else nblocks), (nblocks, first)
        # the kernel's compare, block >= first, raises exactly the last R blocks of a launch that has more than R and none otherwise
        assert nblocks - first == (R if nblocks > R else 0)


def test_a_single_cu(built_lib):
    # 12 streams of 4 per workgroup on one CU: three workgroups resident
    assert [pirip_amd.launch_first_tail_block(n, 12, 4, 1) for n in (0, 1, 3, 4, 6, 100)] == [0, 1, 3, 1, 3, 97]


def test_the_headline_launch(built_lib):
    # bench.py's defaults on 256 CUs: 16384 streams = 4096 workgroups, 768 resident
    assert pirip_amd.launch_first_tail_block(4096, 12, 4, 256) == 3328
    assert pirip_amd.launch_first_tail_block(768, 12, 4, 256) == 768
    assert pirip_amd.launch_first_tail_block(769, 12, 4, 256) == 1


def test_bad_arguments_and_unknown_residency(built_lib):
    L = pirip_amd.lib()
    assert L.pirip_hip_launch_first_tail_block(-1, 12, 4, 256) < 0
    # a device whose CU count could not be read (0), or a shape without an instance: nothing raised
    assert pirip_amd.launch_first_tail_block(5000, 12, 4, 0) == 5000
    assert pirip_amd.launch_first_tail_block(5000, 0, 4, 256) == 5000
    assert pirip_amd.launch_first_tail_block(5000, 12, 0, 256) == 5000
    assert L.pirip_hip_set_launch_tail_first(None, 1) < 0
    assert L.pirip_hip_get_launch_resident_blocks(None) < 0


def test_no_build_rule_defines_the_timing_macro(built_lib):
    """the per-wave timeline (tools/wave_drain.py) is compiled only with EXTRA=-DPIRIP_WAVE_TIMING: its entry point is no symbol of the product"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "PIRIP_WAVE_TIMING" not in open(os.path.join(root, "pirip_amd", "csrc", "Makefile")).read()
    src = open(os.path.join(root, "pirip_amd", "csrc", "fsk_demod_wave.hip")).read()
    i = src.index("int pirip_hip_wave_timeline(")
    assert src.rfind("#ifdef PIRIP_WAVE_TIMING", 0, i) > src.rfind("#endif", 0, i)
    if "timing" not in pirip_amd.lib_path():
        out = subprocess.run(["nm", "-D", "--defined-only", pirip_amd.lib_path()], capture_output=True, text=True, check=True).stdout
        assert "pirip_hip_wave_timeline" not in out
