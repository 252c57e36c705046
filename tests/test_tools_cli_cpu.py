"""The command-line tools' argument checking and no-device behaviour, pinned: every line below was run through the tools as they were
before their host code moved into pirip_amd/tools/tool_common.hpp and tx_records.hpp, and its exit code, stderr and (as a hash) stdout
recorded in EXPECTED. The tools must still answer the same, byte for byte; only argv[0] and the source position in a HIP error
message (HIPOK's file:line, mgpu_receiver's "at line N") are normalised. All lines run in an empty directory that holds a copy of the
stand-in code file, with empty stdin and no PIRIP_* variable but the ones the line sets."""
import hashlib
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "pirip_amd", "bin")
CODE = "standin_256_512_4.code"

RX = ["-s", "240000", "-a", "40000", "-r", "1000"]                                  # D = 6, Ts = 40
TXC = ["--code", CODE] + RX + ["--f1", "1000", "--shift", "2000"]
RPT = TXC + ["--source", "1", "--block", "24000", "-o", "-"]

# (name, tool, arguments, environment); the names are EXPECTED's keys
CASES = [
    ("rtl_fsk/no-args", "rtl_fsk", [], {}),
    ("rtl_fsk/unknown-option", "rtl_fsk", ["--bogus", "-"], {}),
    ("rtl_fsk/no-iq-source", "rtl_fsk", ["-"], {}),
    ("rtl_fsk/m3", "rtl_fsk", ["-i", "-", "-m", "3", "-"], {}),
    ("rtl_fsk/rtl-not-multiple-of-modem", "rtl_fsk", ["-i", "-", "-s", "240000", "-a", "70000", "-"], {}),
    ("rtl_fsk/modem-not-multiple-of-rs", "rtl_fsk", ["-i", "-", "-s", "240000", "-r", "7000", "-"], {}),
    ("rtl_fsk/b-without-code", "rtl_fsk", ["-i", "-", "-b", "-"], {}),
    ("rtl_fsk/testframes-without-code", "rtl_fsk", ["-i", "-", "--testframes", "-"], {}),
    ("rtl_fsk/code-nowhere", "rtl_fsk", ["-i", "-", "--code", "nosuch", "-"], {}),
    ("rtl_fsk/rules-p_rule-9", "rtl_fsk", ["-i", "-", "-"], {"PIRIP_RTL_FSK_RULES": "p_rule=9"}),
    ("rtl_fsk/rules-unknown-key", "rtl_fsk", ["-i", "-", "-"], {"PIRIP_RTL_FSK_RULES": "q=1"}),
    ("rtl_fsk/cannot-open", "rtl_fsk", ["-i", "missing.iq8", "-"], {}),

    ("rtl_fsk_channels/no-args", "rtl_fsk_channels", [], {}),
    ("rtl_fsk_channels/unknown-option", "rtl_fsk_channels", RX + ["-c", "0", "-o", "o", "--bogus"], {}),
    ("rtl_fsk_channels/m3", "rtl_fsk_channels", RX + ["-c", "0", "-o", "o", "-m", "3"], {}),
    ("rtl_fsk_channels/rtl-not-multiple-of-modem", "rtl_fsk_channels", ["-s", "240000", "-a", "70000", "-r", "1000", "-c", "0", "-o", "o"], {}),
    ("rtl_fsk_channels/modem-not-multiple-of-rs", "rtl_fsk_channels", ["-s", "240000", "-a", "40000", "-r", "7000", "-c", "0", "-o", "o"], {}),
    ("rtl_fsk_channels/c-empty-token", "rtl_fsk_channels", RX + ["-c", "1,,2", "-o", "o"], {}),
    ("rtl_fsk_channels/c-trailing-comma", "rtl_fsk_channels", RX + ["-c", "1,", "-o", "o"], {}),
    ("rtl_fsk_channels/c-hex", "rtl_fsk_channels", RX + ["-c", "0x10", "-o", "o"], {}),
    ("rtl_fsk_channels/testframes-without-code", "rtl_fsk_channels", RX + ["-c", "0", "-o", "o", "--testframes"], {}),
    ("rtl_fsk_channels/put-test-bits-with-code", "rtl_fsk_channels", RX + ["-c", "0", "-o", "o", "--put-test-bits", "--code", CODE], {}),
    ("rtl_fsk_channels/code-nowhere", "rtl_fsk_channels", RX + ["-c", "0", "-o", "o", "--code", "nosuch"], {}),
    ("rtl_fsk_channels/cannot-open", "rtl_fsk_channels", RX + ["-c", "0", "-o", "o", "-i", "missing.iq8"], {}),

    ("fsk_ldpc_tx_channels/no-args", "fsk_ldpc_tx_channels", [], {}),
    ("fsk_ldpc_tx_channels/unknown-option", "fsk_ldpc_tx_channels", TXC + ["-c", "0", "--testframes", "1", "-o", "-", "--bogus"], {}),
    ("fsk_ldpc_tx_channels/m3", "fsk_ldpc_tx_channels", TXC + ["-c", "0", "--testframes", "1", "-o", "-", "-m", "3"], {}),
    ("fsk_ldpc_tx_channels/wide-not-multiple-of-modem", "fsk_ldpc_tx_channels",
     ["--code", CODE, "-s", "240000", "-a", "70000", "-r", "1000", "--f1", "1000", "--shift", "2000", "-c", "0", "--testframes", "1", "-o", "-"], {}),
    ("fsk_ldpc_tx_channels/modem-not-multiple-of-rs", "fsk_ldpc_tx_channels",
     ["--code", CODE, "-s", "240000", "-a", "40000", "-r", "7000", "--f1", "1000", "--shift", "2000", "-c", "0", "--testframes", "1", "-o", "-"], {}),
    ("fsk_ldpc_tx_channels/c-empty-token", "fsk_ldpc_tx_channels", TXC + ["-c", "1,,2", "--testframes", "1", "-o", "-"], {}),
    ("fsk_ldpc_tx_channels/gains-wrong-count", "fsk_ldpc_tx_channels", TXC + ["-c", "0,1000,2000", "--gains", "0.1,0.2", "--testframes", "1", "-o", "-"], {}),
    ("fsk_ldpc_tx_channels/gains-junk", "fsk_ldpc_tx_channels", TXC + ["-c", "0", "--gain", "0.1x", "--testframes", "1", "-o", "-"], {}),
    ("fsk_ldpc_tx_channels/gap-1-with-m4", "fsk_ldpc_tx_channels", TXC + ["-c", "0", "-m", "4", "--gap", "1", "--testframes", "1", "-o", "-"], {}),
    ("fsk_ldpc_tx_channels/queue-without-block", "fsk_ldpc_tx_channels", TXC + ["-c", "0", "--queue", "100", "--testframes", "1", "-o", "-"], {}),
    ("fsk_ldpc_tx_channels/lead-with-block", "fsk_ldpc_tx_channels", TXC + ["-c", "0", "--lead", "8", "--block", "24000", "--testframes", "1", "-o", "-"], {}),
    ("fsk_ldpc_tx_channels/block-not-positive", "fsk_ldpc_tx_channels", TXC + ["-c", "0", "--block", "0", "--testframes", "1", "-o", "-"], {}),
    ("fsk_ldpc_tx_channels/source-wrong-count", "fsk_ldpc_tx_channels", TXC + ["-c", "0,1000,2000", "--source", "1,2", "--testframes", "1", "-o", "-"], {}),
    ("fsk_ldpc_tx_channels/source-empty-token", "fsk_ldpc_tx_channels", TXC + ["-c", "0", "--source", ",1", "--testframes", "1", "-o", "-"], {}),
    ("fsk_ldpc_tx_channels/testframes-without-code", "fsk_ldpc_tx_channels", RX + ["--f1", "1000", "--shift", "2000", "-c", "0", "--testframes", "1", "-o", "-"], {}),
    ("fsk_ldpc_tx_channels/code-nowhere", "fsk_ldpc_tx_channels",
     ["--code", "nosuch"] + RX + ["--f1", "1000", "--shift", "2000", "-c", "0", "--testframes", "1", "-o", "-"], {}),
    ("fsk_ldpc_tx_channels/cannot-open-records", "fsk_ldpc_tx_channels", TXC + ["-c", "0", "-i", "missing", "-o", "-"], {}),

    ("frame_repeater_channels/no-args", "frame_repeater_channels", [], {}),
    ("frame_repeater_channels/unknown-option", "frame_repeater_channels", RPT + ["-c", "0", "--bogus"], {}),
    ("frame_repeater_channels/m3", "frame_repeater_channels", RPT + ["-c", "0", "-m", "3"], {}),
    ("frame_repeater_channels/wide-not-multiple-of-modem", "frame_repeater_channels",
     ["--code", CODE, "-s", "240000", "-a", "70000", "-r", "1000", "--f1", "1000", "--shift", "2000", "--source", "1", "--block", "24000", "-o", "-", "-c", "0"], {}),
    ("frame_repeater_channels/modem-not-multiple-of-rs", "frame_repeater_channels",
     ["--code", CODE, "-s", "240000", "-a", "40000", "-r", "7000", "--f1", "1000", "--shift", "2000", "--source", "1", "--block", "24000", "-o", "-", "-c", "0"], {}),
    ("frame_repeater_channels/c-empty-token", "frame_repeater_channels", RPT + ["-c", "1,,2"], {}),
    ("frame_repeater_channels/gains-wrong-count", "frame_repeater_channels", RPT + ["-c", "0,1000,2000", "--gains", "0.1,0.2"], {}),
    ("frame_repeater_channels/route-wrong-count", "frame_repeater_channels", RPT + ["-c", "0,1000,2000", "--route", "0,1"], {}),
    ("frame_repeater_channels/route-junk", "frame_repeater_channels", RPT + ["-c", "0", "--route", "0x"], {}),
    ("frame_repeater_channels/gap-1-with-m4", "frame_repeater_channels", RPT + ["-c", "0", "-m", "4", "--gap", "1"], {}),
    ("frame_repeater_channels/block-not-multiple-of-d-ts", "frame_repeater_channels", TXC + ["--source", "1", "--block", "1000", "-o", "-", "-c", "0"], {}),
    ("frame_repeater_channels/source-300", "frame_repeater_channels", TXC + ["--source", "300", "--block", "24000", "-o", "-", "-c", "0"], {}),
    ("frame_repeater_channels/source-missing", "frame_repeater_channels", TXC + ["--block", "24000", "-o", "-", "-c", "0"], {}),
    ("frame_repeater_channels/holdoff-negative", "frame_repeater_channels", RPT + ["-c", "0", "--holdoff", "-1"], {}),
    ("frame_repeater_channels/code-nowhere", "frame_repeater_channels",
     ["--code", "nosuch"] + RX + ["--f1", "1000", "--shift", "2000", "--source", "1", "--block", "24000", "-o", "-", "-c", "0"], {}),
    ("frame_repeater_channels/cannot-open", "frame_repeater_channels", RPT + ["-c", "0", "-i", "missing.iq8"], {}),

    ("fsk_ldpc_tx/no-args", "fsk_ldpc_tx", [], {}),
    ("fsk_ldpc_tx/unknown-option", "fsk_ldpc_tx", ["--bogus"], {}),
    ("fsk_ldpc_tx/m3", "fsk_ldpc_tx", ["--code", CODE, "-m", "3", "40000", "1000", "1000", "2000", "-", "-"], {}),
    ("fsk_ldpc_tx/fs-not-multiple-of-rs", "fsk_ldpc_tx", ["--code", CODE, "40000", "7000", "1000", "2000", "-", "-"], {}),
    ("fsk_ldpc_tx/gap-1-with-m4", "fsk_ldpc_tx", ["--code", CODE, "-m", "4", "--gap", "1", "40000", "1000", "1000", "2000", "-", "-"], {}),
    ("fsk_ldpc_tx/format", "fsk_ldpc_tx", ["--code", CODE, "--format", "s16", "40000", "1000", "1000", "2000", "-", "-"], {}),
    ("fsk_ldpc_tx/testframes-without-code", "fsk_ldpc_tx", ["--testframes", "1", "40000", "1000", "1000", "2000", "/dev/zero", "-"], {}),
    ("fsk_ldpc_tx/code-nowhere", "fsk_ldpc_tx", ["--code", "nosuch", "40000", "1000", "1000", "2000", "-", "-"], {}),
    ("fsk_ldpc_tx/cannot-open", "fsk_ldpc_tx", ["--code", CODE, "40000", "1000", "1000", "2000", "missing", "-"], {}),

    # the framer needs no device: its output is pinned too (stdout's hash)
    ("fsk_ldpc_framer/no-args", "fsk_ldpc_framer", [], {}),
    ("fsk_ldpc_framer/unknown-option", "fsk_ldpc_framer", ["--bogus"], {}),
    ("fsk_ldpc_framer/m3", "fsk_ldpc_framer", ["--code", CODE, "-m", "3", "-", "-"], {}),
    ("fsk_ldpc_framer/code-nowhere", "fsk_ldpc_framer", ["--code", "nosuch", "-", "-"], {}),
    ("fsk_ldpc_framer/testframes", "fsk_ldpc_framer", ["--code", CODE, "--testframes", "3", "--bursts", "2", "--gap", "16", "/dev/zero", "-"], {}),
    ("fsk_ldpc_framer/testframes-source-seq", "fsk_ldpc_framer", ["--code", CODE, "--testframes", "3", "--source", "0x5", "--seq", "/dev/zero", "-"], {}),
    ("fsk_ldpc_framer/source-300", "fsk_ldpc_framer", ["--code", CODE, "-m", "4", "--testframes", "2", "--source", "300", "/dev/zero", "-"], {}),
    ("fsk_ldpc_framer/empty-input", "fsk_ldpc_framer", ["--code", CODE, "-", "-"], {}),

    ("fsk_demod/no-args", "fsk_demod", [], {}),
    ("fsk_demod/unknown-option", "fsk_demod", ["--bogus"], {}),
    ("fsk_demod/cannot-open", "fsk_demod", ["2", "240000", "10000", "missing", "-"], {}),
    ("csdr/no-args", "csdr", [], {}),
]

# ... and what only a machine without a HIP device answers: one valid line per GPU tool, and the lines whose check sits behind the
# first handle
NO_DEVICE_CASES = [
    ("rtl_fsk/valid", "rtl_fsk", ["-i", "-", "-"], {}),
    ("rtl_fsk/valid-code", "rtl_fsk", ["-i", "-", "--code", CODE, "-a", "40000", "-r", "1000", "-q", "-b", "-"], {}),
    ("rtl_fsk_channels/valid", "rtl_fsk_channels", RX + ["-c", "-90000,30001", "-o", "o"], {}),
    # rtl_fsk_channels borrows rtl_fsk's modem settings but not its environment switch: were it read, p_rule=9 would be refused
    ("rtl_fsk_channels/valid-ignores-rules", "rtl_fsk_channels", RX + ["-c", "-90000,30001", "-o", "o"], {"PIRIP_RTL_FSK_RULES": "p_rule=1"}),
    ("rtl_fsk_channels/ignores-bad-rules", "rtl_fsk_channels", RX + ["-c", "-90000,30001", "-o", "o"], {"PIRIP_RTL_FSK_RULES": "p_rule=9"}),
    ("frame_repeater_channels/valid", "frame_repeater_channels", RPT + ["-c", "-90000,30001"], {}),
    ("frame_repeater_channels/ignores-bad-rules", "frame_repeater_channels", RPT + ["-c", "-90000,30001"], {"PIRIP_RTL_FSK_RULES": "p_rule=9"}),
    ("fsk_ldpc_tx_channels/valid", "fsk_ldpc_tx_channels", TXC + ["-c", "-90000,30001", "--testframes", "2", "--seq", "--source", "1,2", "-o", "-"], {}),
    ("fsk_ldpc_tx_channels/block-not-multiple-of-d-ts", "fsk_ldpc_tx_channels", TXC + ["-c", "0", "--block", "1000", "--testframes", "1", "-o", "-"], {}),
    ("fsk_ldpc_tx_channels/source-300", "fsk_ldpc_tx_channels", TXC + ["-c", "0", "--source", "300", "--testframes", "1", "-o", "-"], {}),
    ("fsk_ldpc_tx/valid", "fsk_ldpc_tx", ["--code", CODE, "--testframes", "2", "--bursts", "2", "40000", "1000", "1000", "2000", "/dev/zero", "-"], {}),
    ("fsk_ldpc_tx/source-300", "fsk_ldpc_tx", ["--code", CODE, "--testframes", "1", "--source", "300", "40000", "1000", "1000", "2000", "/dev/zero", "-"], {}),
    ("fsk_demod/valid", "fsk_demod", ["-d", "-p", "24", "2", "240000", "10000", "-", "-"], {}),
    ("csdr/valid", "csdr", ["convert_u8_f"], {}),
    ("csdr/unknown-function", "csdr", ["bogus"], {}),
    ("mgpu_receiver/valid", "mgpu_receiver", ["--streams", "2", "--samples", "12000", "--steps", "1", "--warmup", "0", "--id-file", "id"], {}),
]


def run_case(bin_dir, workdir, tool, args, env_extra):
    """(exit code, normalised stderr, sha256 of stdout) of one line."""
    exe = os.path.join(bin_dir, tool)
    env = {k: v for k, v in os.environ.items() if not k.startswith("PIRIP_")}
    env.update(env_extra)
    p = subprocess.run([exe] + args, cwd=workdir, env=env, stdin=subprocess.DEVNULL, capture_output=True, timeout=60)
    err = p.stderr.decode().replace(exe, tool)
    err = re.sub(r"HIP error at \S+:\d+", "HIP error at FILE:LINE", err)
    err = re.sub(r"(mgpu_receiver\[\d+\]: .* failed at line )\d+", r"\1N", err)
    return p.returncode, err, hashlib.sha256(p.stdout).hexdigest()


NO_OUTPUT = hashlib.sha256(b"").hexdigest()

# (exit code, stderr, sha256 of stdout), as recorded from the tools before the change on a machine without a HIP device
EXPECTED = {
    'rtl_fsk/no-args': (1,
        'rtl_fsk (pirip_hip): [-i <u8 IQ file|->] [-s rtlFs] [-a modemFs] [-r Rs] [-m M] [-n nSamples] [--mask spacing]\n'
        '        [-l fsk_lower] [-U fsk_upper] [--code NAME|FILE [--filter addr] [--testframes] [-b]] [-u dashHost] [-v] [-q] <out|->\n'
        '        IQ source: -i, or the file named by $PIRIP_IQ_FILE; tuner options -g -f -w -e -p are accepted and ignored\n',
        NO_OUTPUT),
    'rtl_fsk/unknown-option': (1,
        "rtl_fsk: unrecognized option '--bogus'\n"
        'rtl_fsk (pirip_hip): [-i <u8 IQ file|->] [-s rtlFs] [-a modemFs] [-r Rs] [-m M] [-n nSamples] [--mask spacing]\n'
        '        [-l fsk_lower] [-U fsk_upper] [--code NAME|FILE [--filter addr] [--testframes] [-b]] [-u dashHost] [-v] [-q] <out|->\n'
        '        IQ source: -i, or the file named by $PIRIP_IQ_FILE; tuner options -g -f -w -e -p are accepted and ignored\n',
        NO_OUTPUT),
    'rtl_fsk/no-iq-source': (2,
        'rtl_fsk: no RTL-SDR hardware support in this build; give the 8-bit IQ with -i FILE, -i - or $PIRIP_IQ_FILE\n',
        NO_OUTPUT),
    'rtl_fsk/m3': (2,
        'rtl_fsk: bad modem configuration (codec2 fsk_create would assert) (AMD GPU only; there is no CPU fallback)\n',
        NO_OUTPUT),
    'rtl_fsk/rtl-not-multiple-of-modem': (1,
        'rtl_fsk: rtl rate 240000 must be a multiple of the modem rate 70000\n',
        NO_OUTPUT),
    'rtl_fsk/modem-not-multiple-of-rs': (1,
        'rtl_fsk: modem rate must be a multiple of the symbol rate\n',
        NO_OUTPUT),
    'rtl_fsk/b-without-code': (1,
        'rtl_fsk: -b / --testframes / --filter need --code\n',
        NO_OUTPUT),
    'rtl_fsk/testframes-without-code': (1,
        'rtl_fsk: -b / --testframes / --filter need --code\n',
        NO_OUTPUT),
    'rtl_fsk/code-nowhere': (2,
        "rtl_fsk: no table for --code nosuch: codec2's LDPC tables are not part of this build (SURVEY.md 7.6);\n"
        '         drop nosuch.code (format: pirip_amd/csrc/fsk_ldpc.hpp) into $PIRIP_CODE_DIR or pass a file path\n',
        NO_OUTPUT),
    'rtl_fsk/rules-p_rule-9': (2,
        'rtl_fsk: PIRIP_RTL_FSK_RULES: unknown key or value out of range\n',
        NO_OUTPUT),
    'rtl_fsk/rules-unknown-key': (2,
        'rtl_fsk: PIRIP_RTL_FSK_RULES: unknown key or value out of range\n',
        NO_OUTPUT),
    'rtl_fsk/cannot-open': (1,
        "rtl_fsk: couldn't open files\n",
        NO_OUTPUT),
    'rtl_fsk_channels/no-args': (1,
        'rtl_fsk_channels (pirip_hip): -s rtlFs -a modemFs -r Rs [-m M] [--mask spacing] [--fsk_lower Hz] [--fsk_upper Hz]\n'
        '        [--code NAME|FILE] -c off1,off2,... [-i <u8 IQ file|->] -o PREFIX [-q]\n'
        '        [--put-test-bits [-p packetsPass] [-b berPass] [-t validBER] [-f frameBits]] [--testframes (with --code)]\n'
        '        writes PREFIX.<k> per channel: bits one per byte, or with --code the payload bytes of every CRC-ok frame\n',
        NO_OUTPUT),
    'rtl_fsk_channels/unknown-option': (1,
        "rtl_fsk_channels: unrecognized option '--bogus'\n"
        'rtl_fsk_channels (pirip_hip): -s rtlFs -a modemFs -r Rs [-m M] [--mask spacing] [--fsk_lower Hz] [--fsk_upper Hz]\n'
        '        [--code NAME|FILE] -c off1,off2,... [-i <u8 IQ file|->] -o PREFIX [-q]\n'
        '        [--put-test-bits [-p packetsPass] [-b berPass] [-t validBER] [-f frameBits]] [--testframes (with --code)]\n'
        '        writes PREFIX.<k> per channel: bits one per byte, or with --code the payload bytes of every CRC-ok frame\n',
        NO_OUTPUT),
    'rtl_fsk_channels/m3': (1,
        'rtl_fsk_channels (pirip_hip): -s rtlFs -a modemFs -r Rs [-m M] [--mask spacing] [--fsk_lower Hz] [--fsk_upper Hz]\n'
        '        [--code NAME|FILE] -c off1,off2,... [-i <u8 IQ file|->] -o PREFIX [-q]\n'
        '        [--put-test-bits [-p packetsPass] [-b berPass] [-t validBER] [-f frameBits]] [--testframes (with --code)]\n'
        '        writes PREFIX.<k> per channel: bits one per byte, or with --code the payload bytes of every CRC-ok frame\n',
        NO_OUTPUT),
    'rtl_fsk_channels/rtl-not-multiple-of-modem': (1,
        'rtl_fsk_channels: rtl rate 240000 must be a multiple of the modem rate 70000\n',
        NO_OUTPUT),
    'rtl_fsk_channels/modem-not-multiple-of-rs': (1,
        'rtl_fsk_channels: modem rate must be a multiple of the symbol rate\n',
        NO_OUTPUT),
    'rtl_fsk_channels/c-empty-token': (1,
        'rtl_fsk_channels: -c wants integer offsets in Hz, comma separated\n',
        NO_OUTPUT),
    'rtl_fsk_channels/c-trailing-comma': (1,
        'rtl_fsk_channels: -c wants integer offsets in Hz, comma separated\n',
        NO_OUTPUT),
    'rtl_fsk_channels/c-hex': (1,
        'rtl_fsk_channels: -c wants integer offsets in Hz, comma separated\n',
        NO_OUTPUT),
    'rtl_fsk_channels/testframes-without-code': (1,
        'rtl_fsk_channels: --testframes needs --code\n',
        NO_OUTPUT),
    'rtl_fsk_channels/put-test-bits-with-code': (1,
        'rtl_fsk_channels: --put-test-bits counts uncoded bits; with --code use --testframes\n',
        NO_OUTPUT),
    'rtl_fsk_channels/code-nowhere': (2,
        'rtl_fsk_channels: no table for --code nosuch (format: pirip_amd/csrc/fsk_ldpc.hpp; $PIRIP_CODE_DIR or a file path)\n',
        NO_OUTPUT),
    'rtl_fsk_channels/cannot-open': (1,
        "rtl_fsk_channels: can't open missing.iq8\n",
        NO_OUTPUT),
    'fsk_ldpc_tx_channels/no-args': (1,
        'usage: fsk_ldpc_tx_channels --code NAME|FILE -s wideFs -a modemFs -r Rs [-m 2|4] --f1 Hz --shift Hz -c off1,off2,...\n'
        '          [--gain g | --gains g1,g2,...] [--linear] [--format u8|cf32] [--packed] [--gap BITS] [--lead BITS]\n'
        '          [--testframes N [--bursts B] [--seq] [--source BYTE|b1,b2,...]] [--block N [--queue SYMS]] -i PREFIX -o out|-\n',
        NO_OUTPUT),
    'fsk_ldpc_tx_channels/unknown-option': (1,
        "fsk_ldpc_tx_channels: unrecognized option '--bogus'\n"
        'usage: fsk_ldpc_tx_channels --code NAME|FILE -s wideFs -a modemFs -r Rs [-m 2|4] --f1 Hz --shift Hz -c off1,off2,...\n'
        '          [--gain g | --gains g1,g2,...] [--linear] [--format u8|cf32] [--packed] [--gap BITS] [--lead BITS]\n'
        '          [--testframes N [--bursts B] [--seq] [--source BYTE|b1,b2,...]] [--block N [--queue SYMS]] -i PREFIX -o out|-\n',
        NO_OUTPUT),
    'fsk_ldpc_tx_channels/m3': (1,
        'usage: fsk_ldpc_tx_channels --code NAME|FILE -s wideFs -a modemFs -r Rs [-m 2|4] --f1 Hz --shift Hz -c off1,off2,...\n'
        '          [--gain g | --gains g1,g2,...] [--linear] [--format u8|cf32] [--packed] [--gap BITS] [--lead BITS]\n'
        '          [--testframes N [--bursts B] [--seq] [--source BYTE|b1,b2,...]] [--block N [--queue SYMS]] -i PREFIX -o out|-\n',
        NO_OUTPUT),
    'fsk_ldpc_tx_channels/wide-not-multiple-of-modem': (1,
        'fsk_ldpc_tx_channels: the wideband rate 240000 must be a multiple of the modem rate 70000\n',
        NO_OUTPUT),
    'fsk_ldpc_tx_channels/modem-not-multiple-of-rs': (1,
        'fsk_ldpc_tx_channels: need modemFs % Rs == 0 and --shift > 0\n',
        NO_OUTPUT),
    'fsk_ldpc_tx_channels/c-empty-token': (1,
        'fsk_ldpc_tx_channels: -c wants integer offsets in Hz, comma separated\n',
        NO_OUTPUT),
    'fsk_ldpc_tx_channels/gains-wrong-count': (1,
        'fsk_ldpc_tx_channels: one gain, or one per channel\n',
        NO_OUTPUT),
    'fsk_ldpc_tx_channels/gains-junk': (1,
        'fsk_ldpc_tx_channels: --gain g or --gains g1,g2,...\n',
        NO_OUTPUT),
    'fsk_ldpc_tx_channels/gap-1-with-m4': (1,
        'fsk_ldpc_tx_channels: --gap / --lead are whole symbols, --bursts >= 1, --testframes >= 0\n',
        NO_OUTPUT),
    'fsk_ldpc_tx_channels/queue-without-block': (1,
        'fsk_ldpc_tx_channels: --queue needs --block\n',
        NO_OUTPUT),
    'fsk_ldpc_tx_channels/lead-with-block': (1,
        "fsk_ldpc_tx_channels: --lead does not go with --block: a streaming transmitter's silence is its empty queue\n",
        NO_OUTPUT),
    'fsk_ldpc_tx_channels/block-not-positive': (1,
        'fsk_ldpc_tx_channels: --block wants a positive number of wideband samples\n',
        NO_OUTPUT),
    'fsk_ldpc_tx_channels/source-wrong-count': (1,
        'fsk_ldpc_tx_channels: one --source byte, or one per channel\n',
        NO_OUTPUT),
    'fsk_ldpc_tx_channels/source-empty-token': (1,
        'fsk_ldpc_tx_channels: --source BYTE or b1,b2,...\n',
        NO_OUTPUT),
    'fsk_ldpc_tx_channels/testframes-without-code': (1,
        'usage: fsk_ldpc_tx_channels --code NAME|FILE -s wideFs -a modemFs -r Rs [-m 2|4] --f1 Hz --shift Hz -c off1,off2,...\n'
        '          [--gain g | --gains g1,g2,...] [--linear] [--format u8|cf32] [--packed] [--gap BITS] [--lead BITS]\n'
        '          [--testframes N [--bursts B] [--seq] [--source BYTE|b1,b2,...]] [--block N [--queue SYMS]] -i PREFIX -o out|-\n',
        NO_OUTPUT),
    'fsk_ldpc_tx_channels/code-nowhere': (2,
        'fsk_ldpc_tx_channels: no table for --code nosuch (format: pirip_amd/csrc/fsk_ldpc.hpp; $PIRIP_CODE_DIR or a file path)\n',
        NO_OUTPUT),
    'fsk_ldpc_tx_channels/cannot-open-records': (1,
        "fsk_ldpc_tx_channels: couldn't open missing.0\n",
        NO_OUTPUT),
    'frame_repeater_channels/no-args': (1,
        'frame_repeater_channels (pirip_hip): --code NAME|FILE -s wideFs -a modemFs -r Rs [-m M] [--mask spacing] [--fsk_lower Hz] [--fsk_upper Hz]\n'
        '        -c off1,off2,... --f1 Hz --shift Hz [--gain g | --gains g1,g2,...] [--linear] [--gap BITS] --block N [--queue SYMS]\n'
        '        --source A [--filter A] [--route a,b,...] [--holdoff N] [--max-burst N] [--pending RECORDS] [-i <u8 IQ file|->] -o <file|-> [-q]\n',
        NO_OUTPUT),
    'frame_repeater_channels/unknown-option': (1,
        "frame_repeater_channels: unrecognized option '--bogus'\n"
        'frame_repeater_channels (pirip_hip): --code NAME|FILE -s wideFs -a modemFs -r Rs [-m M] [--mask spacing] [--fsk_lower Hz] [--fsk_upper Hz]\n'
        '        -c off1,off2,... --f1 Hz --shift Hz [--gain g | --gains g1,g2,...] [--linear] [--gap BITS] --block N [--queue SYMS]\n'
        '        --source A [--filter A] [--route a,b,...] [--holdoff N] [--max-burst N] [--pending RECORDS] [-i <u8 IQ file|->] -o <file|-> [-q]\n',
        NO_OUTPUT),
    'frame_repeater_channels/m3': (1,
        'frame_repeater_channels (pirip_hip): --code NAME|FILE -s wideFs -a modemFs -r Rs [-m M] [--mask spacing] [--fsk_lower Hz] [--fsk_upper Hz]\n'
        '        -c off1,off2,... --f1 Hz --shift Hz [--gain g | --gains g1,g2,...] [--linear] [--gap BITS] --block N [--queue SYMS]\n'
        '        --source A [--filter A] [--route a,b,...] [--holdoff N] [--max-burst N] [--pending RECORDS] [-i <u8 IQ file|->] -o <file|-> [-q]\n',
        NO_OUTPUT),
    'frame_repeater_channels/wide-not-multiple-of-modem': (1,
        'frame_repeater_channels: the wideband rate 240000 must be a multiple of the modem rate 70000\n',
        NO_OUTPUT),
    'frame_repeater_channels/modem-not-multiple-of-rs': (1,
        'frame_repeater_channels: need modemFs % Rs == 0 and --shift > 0\n',
        NO_OUTPUT),
    'frame_repeater_channels/c-empty-token': (1,
        'frame_repeater_channels: -c wants integer offsets in Hz, comma separated\n',
        NO_OUTPUT),
    'frame_repeater_channels/gains-wrong-count': (1,
        'frame_repeater_channels: one gain, or one per channel\n',
        NO_OUTPUT),
    'frame_repeater_channels/route-wrong-count': (1,
        'frame_repeater_channels: --route wants 3 entries, one per channel\n',
        NO_OUTPUT),
    'frame_repeater_channels/route-junk': (1,
        'frame_repeater_channels: --route wants one transmit channel per receive channel, -1 = none\n',
        NO_OUTPUT),
    'frame_repeater_channels/gap-1-with-m4': (1,
        'frame_repeater_channels: --gap is whole symbols\n',
        NO_OUTPUT),
    'frame_repeater_channels/block-not-multiple-of-d-ts': (1,
        'frame_repeater_channels: --block must be a multiple of D * Ts = 240 wideband samples\n',
        NO_OUTPUT),
    'frame_repeater_channels/source-300': (1,
        'frame_repeater_channels: --source A (0 .. 255) is needed; --filter A likewise\n',
        NO_OUTPUT),
    'frame_repeater_channels/source-missing': (1,
        'frame_repeater_channels: --source A (0 .. 255) is needed; --filter A likewise\n',
        NO_OUTPUT),
    'frame_repeater_channels/holdoff-negative': (1,
        'frame_repeater_channels: --holdoff >= 0, --max-burst 1 .. 100\n',
        NO_OUTPUT),
    'frame_repeater_channels/code-nowhere': (2,
        'frame_repeater_channels: no table for --code nosuch (format: pirip_amd/csrc/fsk_ldpc.hpp; $PIRIP_CODE_DIR or a file path)\n',
        NO_OUTPUT),
    'frame_repeater_channels/cannot-open': (1,
        "frame_repeater_channels: can't open missing.iq8\n",
        NO_OUTPUT),
    'fsk_ldpc_tx/no-args': (1,
        'fsk_ldpc_tx: need --code FILE, -m 2|4, Fs Rs f1 shift, input and output\n'
        'usage: fsk_ldpc_tx --code FILE [-m 2|4] [--packed] [--testframes N [--bursts B]] [--source BYTE] [--seq] [--gap BITS] [--lead BITS]\n'
        '          [--format u8|cf32] [--amp A] Fs Rs f1 shift in|- out|-\n',
        NO_OUTPUT),
    'fsk_ldpc_tx/unknown-option': (1,
        "fsk_ldpc_tx: unrecognized option '--bogus'\n"
        'usage: fsk_ldpc_tx --code FILE [-m 2|4] [--packed] [--testframes N [--bursts B]] [--source BYTE] [--seq] [--gap BITS] [--lead BITS]\n'
        '          [--format u8|cf32] [--amp A] Fs Rs f1 shift in|- out|-\n',
        NO_OUTPUT),
    'fsk_ldpc_tx/m3': (1,
        'fsk_ldpc_tx: need --code FILE, -m 2|4, Fs Rs f1 shift, input and output\n'
        'usage: fsk_ldpc_tx --code FILE [-m 2|4] [--packed] [--testframes N [--bursts B]] [--source BYTE] [--seq] [--gap BITS] [--lead BITS]\n'
        '          [--format u8|cf32] [--amp A] Fs Rs f1 shift in|- out|-\n',
        NO_OUTPUT),
    'fsk_ldpc_tx/fs-not-multiple-of-rs': (1,
        'fsk_ldpc_tx: need Fs > 0, Rs > 0, Fs % Rs == 0 and shift > 0\n',
        NO_OUTPUT),
    'fsk_ldpc_tx/gap-1-with-m4': (1,
        'fsk_ldpc_tx: --gap / --lead are whole symbols, --bursts >= 1\n',
        NO_OUTPUT),
    'fsk_ldpc_tx/format': (1,
        'fsk_ldpc_tx: --format u8|cf32\n',
        NO_OUTPUT),
    'fsk_ldpc_tx/testframes-without-code': (1,
        'fsk_ldpc_tx: need --code FILE, -m 2|4, Fs Rs f1 shift, input and output\n'
        'usage: fsk_ldpc_tx --code FILE [-m 2|4] [--packed] [--testframes N [--bursts B]] [--source BYTE] [--seq] [--gap BITS] [--lead BITS]\n'
        '          [--format u8|cf32] [--amp A] Fs Rs f1 shift in|- out|-\n',
        NO_OUTPUT),
    'fsk_ldpc_tx/code-nowhere': (2,
        'fsk_ldpc_tx: nosuch: cannot open nosuch\n',
        NO_OUTPUT),
    'fsk_ldpc_tx/cannot-open': (1,
        "fsk_ldpc_tx: couldn't open the input\n",
        NO_OUTPUT),
    'fsk_ldpc_framer/no-args': (1,
        'fsk_ldpc_framer: need --code FILE, -m 2|4, input and output\n',
        NO_OUTPUT),
    'fsk_ldpc_framer/unknown-option': (1,
        "fsk_ldpc_framer: unrecognized option '--bogus'\n"
        'usage: fsk_ldpc_framer --code FILE [-m 2|4] [--packed] [--testframes N [--bursts B]] [--source BYTE] [--seq] [--gap BITS] in|- out|-\n',
        NO_OUTPUT),
    'fsk_ldpc_framer/m3': (1,
        'fsk_ldpc_framer: need --code FILE, -m 2|4, input and output\n',
        NO_OUTPUT),
    'fsk_ldpc_framer/code-nowhere': (2,
        'fsk_ldpc_framer: nosuch: cannot open nosuch\n',
        NO_OUTPUT),
    'fsk_ldpc_framer/testframes': (0,
        'fsk_ldpc_framer: code STANDIN_256_512_4 data_bits_per_frame 256 bits_per_frame 544 M 2\n'
        'fsk_ldpc_framer: End of burst 0\n'
        'fsk_ldpc_framer: End of burst 1\n',
        '490b7117d289e3aa29dfba83e0f6d58c1bbdcda86fdde300e763f36a554065c0'),
    'fsk_ldpc_framer/testframes-source-seq': (0,
        'fsk_ldpc_framer: code STANDIN_256_512_4 data_bits_per_frame 256 bits_per_frame 544 M 2\n'
        'fsk_ldpc_framer: End of burst 0\n',
        'a07a9423e699813cf3eb08ca397b7e8b3b0e6945410519c0822edd5e8d364ab8'),
    'fsk_ldpc_framer/source-300': (0,
        'fsk_ldpc_framer: code STANDIN_256_512_4 data_bits_per_frame 256 bits_per_frame 544 M 4\n'
        'fsk_ldpc_framer: End of burst 0\n',
        '98dbac9c4aa23472aafccc185710cbe1ef13d96596245b09a5a59331788a11d8'),
    'fsk_ldpc_framer/empty-input': (0,
        'fsk_ldpc_framer: code STANDIN_256_512_4 data_bits_per_frame 256 bits_per_frame 544 M 2\n',
        NO_OUTPUT),
    'fsk_demod/no-args': (1,
        'Too few arguments\n',
        NO_OUTPUT),
    'fsk_demod/unknown-option': (1,
        "fsk_demod: unrecognized option '--bogus'\n"
        'usage: fsk_demod [--fsk_lower Hz] [--fsk_upper Hz] [-d|-c] [-p P] [--mask spacing] [-s] M Fs Rs in out\n',
        NO_OUTPUT),
    'fsk_demod/cannot-open': (1,
        "Couldn't open files\n",
        NO_OUTPUT),
    'csdr/no-args': (255,
        'csdr: need a function name (convert_u8_f | fir_decimate_cc | convert_f_s16)\n',
        NO_OUTPUT),
    'rtl_fsk/valid': (2,
        'rtl_fsk: no usable HIP device (AMD GPU only; there is no CPU fallback)\n',
        NO_OUTPUT),
    'rtl_fsk/valid-code': (2,
        'rtl_fsk: no usable HIP device (AMD GPU only; there is no CPU fallback)\n',
        NO_OUTPUT),
    'rtl_fsk_channels/valid': (2,
        'rtl_fsk_channels: channelizer: no usable HIP device\n',
        NO_OUTPUT),
    'rtl_fsk_channels/valid-ignores-rules': (2,
        'rtl_fsk_channels: channelizer: no usable HIP device\n',
        NO_OUTPUT),
    'rtl_fsk_channels/ignores-bad-rules': (2,
        'rtl_fsk_channels: channelizer: no usable HIP device\n',
        NO_OUTPUT),
    'frame_repeater_channels/valid': (2,
        'frame_repeater_channels: channelizer: no usable HIP device\n',
        NO_OUTPUT),
    'frame_repeater_channels/ignores-bad-rules': (2,
        'frame_repeater_channels: channelizer: no usable HIP device\n',
        NO_OUTPUT),
    'fsk_ldpc_tx_channels/valid': (3,
        'fsk_ldpc_tx_channels: pirip_hip_tx_create: no usable HIP device\n',
        NO_OUTPUT),
    'fsk_ldpc_tx_channels/block-not-multiple-of-d-ts': (3,
        'fsk_ldpc_tx_channels: pirip_hip_tx_create: no usable HIP device\n',
        NO_OUTPUT),
    'fsk_ldpc_tx_channels/source-300': (3,
        'fsk_ldpc_tx_channels: pirip_hip_tx_create: no usable HIP device\n',
        NO_OUTPUT),
    'fsk_ldpc_tx/valid': (3,
        'fsk_ldpc_tx: code STANDIN_256_512_4 data_bits_per_frame 256 bits_per_frame 544 M 2 records 6\n'
        'fsk_ldpc_tx: pirip_hip_tx_create: no usable HIP device\n',
        NO_OUTPUT),
    'fsk_ldpc_tx/source-300': (3,
        'fsk_ldpc_tx: code STANDIN_256_512_4 data_bits_per_frame 256 bits_per_frame 544 M 2 records 2\n'
        'fsk_ldpc_tx: pirip_hip_tx_create: no usable HIP device\n',
        NO_OUTPUT),
    'fsk_demod/valid': (2,
        'Setting estimator limits to -120000 to 120000 Hz.\n'
        'fsk_demod: no usable HIP device (this build demodulates on an AMD GPU only; there is no CPU fallback)\n',
        NO_OUTPUT),
    'csdr/valid': (2,
        'csdr: no usable HIP device (this build runs on an AMD GPU only; there is no CPU fallback)\n',
        NO_OUTPUT),
    'csdr/unknown-function': (2,
        'csdr: no usable HIP device (this build runs on an AMD GPU only; there is no CPU fallback)\n',
        NO_OUTPUT),
    'mgpu_receiver/valid': (2,
        'mgpu_receiver[0]: hipSetDevice(local) failed at line N\n',
        NO_OUTPUT),
}


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    d = tmp_path_factory.mktemp("cli")
    shutil.copy(os.path.join(ROOT, "pirip_amd", "data", CODE), d)
    return str(d)


def test_the_table_covers_every_line():
    names = [c[0] for c in CASES + NO_DEVICE_CASES]
    assert len(set(names)) == len(names) and set(names) == set(EXPECTED)


@pytest.mark.parametrize("name,tool,args,env", CASES, ids=[c[0] for c in CASES])
def test_arguments_are_answered_as_before(built_lib, workdir, name, tool, args, env):
    assert run_case(BIN, workdir, tool, args, env) == EXPECTED[name]


@pytest.mark.parametrize("name,tool,args,env", NO_DEVICE_CASES, ids=[c[0] for c in NO_DEVICE_CASES])
def test_no_device_is_answered_as_before(built_lib, workdir, name, tool, args, env):
    import pirip_amd
    if pirip_amd.device_count() > 0:
        pytest.skip("a HIP device is present")
    assert run_case(BIN, workdir, tool, args, env) == EXPECTED[name]
