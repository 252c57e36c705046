"""pirip_amd/binding.py against include/pirip_hip.h, without a device: the header is the only statement of the C ABI, and ctypes checks
nothing -- a wrong arity or an int where the header says int64_t is silent until a result is wrong.

  * every prototype of the header has one entry in binding.SIGNATURES, of the same arity, each parameter and the return value of the same
    kind (pointer / integer of a size and signedness / float); lib() has applied the table to the loaded library, and no other file of
    the package, the tests or the tools declares a pirip_hip_* function again;
  * every structure the header defines has a twin in the binding -- a ctypes Structure, or for the two record types that numpy reads a
    structured dtype -- with the size, field names, order, offsets and field sizes a C compiler gives the header's;
  * the public surface: tests/golden/binding_api.json holds the public names of pirip_amd and the signatures of its public functions,
    classes and methods as they were before the binding was refactored. Names and signatures may be added, none changed or removed.
    The file was written on that tree by
        import inspect, json, pirip_amd
        def sig(o):
            try: return str(inspect.signature(o))
            except (TypeError, ValueError): return None
        names = sorted(n for n in vars(pirip_amd) if not n.startswith("_") and not inspect.ismodule(getattr(pirip_amd, n)))
        sigs = {}
        for n in names:
            o = getattr(pirip_amd, n)
            if inspect.isclass(o):
                sigs[n] = sig(o)
                sigs.update({f"{n}.{m}": sig(f) for m, f in inspect.getmembers(o, inspect.isfunction) if not m.startswith("_")})
            elif inspect.isfunction(o):
                sigs[n] = sig(o)
        json.dump({"names": names, "signatures": sigs}, open("tests/golden/binding_api.json", "w"), indent=1, sort_keys=True)
    (public_api() below is the same code)."""
import ctypes as C
import inspect
import json
import os
import re
import subprocess

import numpy as np
import pytest

import pirip_amd
from pirip_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pirip_hip.h")


def _header():
    """the header without its comments"""
    src = open(HEADER).read()
    return re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", src, flags=re.S))


def _prototypes():
    """name -> (return type, [parameter declarations]) of every `... pirip_hip_NAME(...);`"""
    out = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w \t\*]*?)\b(pirip_hip_\w+)\s*\(([^()]*)\)\s*;", _header()):
        params = " ".join(params.split())
        assert name not in out, name
        out[name] = (" ".join(ret.split()), [] if params == "void" else [p.strip() for p in params.split(",")])
    return out


C_KINDS = {"int": ("int", 4, True), "int32_t": ("int", 4, True), "int64_t": ("int", 8, True), "size_t": ("int", 8, False),
           "uint64_t": ("int", 8, False), "float": ("float", 4)}


def _c_kind(decl, named=True):
    """the kind of a C parameter declaration (or, named=False, of a bare return type)"""
    if "*" in decl or "[" in decl:
        return ("pointer",)
    words = [w for w in decl.split() if w != "const"]
    assert len(words) == (2 if named else 1), decl
    return C_KINDS[words[0]]


def _ctypes_kind(t):
    """the same of a ctypes type: by size and class, c_size_t / c_uint64 / c_ulong being one type here"""
    if t in (C.c_void_p, C.c_char_p) or issubclass(t, C._Pointer):
        return ("pointer",)
    assert issubclass(t, C._SimpleCData), t
    if t in (C.c_float, C.c_double):
        return ("float", C.sizeof(t))
    assert isinstance(t(0).value, int), t
    return ("int", C.sizeof(t), t(-1).value == -1)


def test_the_table_names_every_prototype_of_the_header():
    protos = _prototypes()
    assert len(protos) >= 149
    assert set(binding.SIGNATURES) == set(protos), sorted(set(binding.SIGNATURES) ^ set(protos))


@pytest.mark.parametrize("name", sorted(_prototypes()))
def test_signature_matches_the_prototype(name):
    ret, params = _prototypes()[name]
    restype, argtypes = binding.SIGNATURES[name]
    assert len(argtypes) == len(params), (name, params, argtypes)
    for i, (decl, t) in enumerate(zip(params, argtypes)):
        assert _ctypes_kind(t) == _c_kind(decl), (name, i, decl, t)
    if ret == "void":
        assert restype is None
    elif ret == "const char *":
        assert restype is C.c_char_p
    elif ret == "int64_t":
        assert restype is C.c_int64
    else:
        assert ret == "int" and _ctypes_kind(restype) == ("int", 4, True), (name, ret, restype)


def test_the_return_types_the_header_has():
    rets = {}
    for name, (ret, _) in _prototypes().items():
        rets.setdefault(ret, []).append(name)
    assert set(rets) == {"int", "int64_t", "const char *", "void"}
    assert len(rets["int64_t"]) == 6 and len(rets["const char *"]) == 3 and rets["void"] == ["pirip_hip_recalled_defaults"]


def test_lib_applies_the_table_to_every_entry_point(built_lib):
    for name, (restype, argtypes) in binding.SIGNATURES.items():
        fn = getattr(built_lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    assert built_lib.pirip_hip_version().decode() and len(pirip_amd.kernel_source_hash()) == 16


def test_a_symbol_the_library_lacks_is_an_error_that_names_it(built_lib, monkeypatch):
    monkeypatch.setitem(binding.SIGNATURES, "pirip_hip_no_such_entry_point", (C.c_int, []))
    monkeypatch.setattr(binding, "_lib", None)
    with pytest.raises(pirip_amd.PiripError, match="pirip_hip_no_such_entry_point"):
        binding.lib()
    assert binding._lib is None


def test_no_other_file_declares_an_entry_point_again():
    """an entry point's argtypes or restype attribute named outside lib(): tools/wave_drain.py's pirip_hip_wave_timeline alone, which
    exists only in -DPIRIP_WAVE_TIMING builds and is deliberately not in the header"""
    found = []
    for top in ("pirip_amd", "tests", "tools"):
        for d, _, files in os.walk(os.path.join(ROOT, top)):
            for f in files:
                if f.endswith((".py", ".sh")):
                    text = open(os.path.join(d, f), errors="replace").read()
                    found += [(os.path.relpath(os.path.join(d, f), ROOT), m.group(1))
                              for m in re.finditer(r"(pirip_hip_\w*)\.(argtypes|restype)", text)]
    assert found == [(os.path.join("tools", "wave_drain.py"), "pirip_hip_wave_timeline")], found


# ---------------------------------------------------------------- structure layouts

TWINS = {
    "pirip_fsk_params": binding.FskParams, "pirip_fsk_info": binding.FskInfo, "pirip_fsk_recalled": binding.FskRecalled,
    "pirip_capture_report": binding.CaptureReport, "pirip_stream_state": binding.StreamState, "pirip_ldpc_info": binding.LdpcInfo,
    "pirip_chain_group": binding.ChainGroup, "pirip_chan_info": binding.ChanInfo, "pirip_tx_info": binding.TxInfo,
    "pirip_mux_info": binding.MuxInfo, "pirip_txs_info": binding.TxsInfo, "pirip_rpt_info": binding.RptInfo,
    "pirip_ping_config": binding.PingConfig, "pirip_ping_entry": binding.PingEntry, "pirip_ping_info": binding.PingInfo,
    "pirip_air_path": binding.AirPath, "pirip_air_info": binding.AirInfo, "pirip_air_path_ex": binding.AirPathEx,
    "pirip_air_fade": binding.AirFade, "pirip_spec_band": binding.SpecBand, "pirip_spec_info": binding.SpecInfo,
}
DTYPES = {"pirip_ping_entry": binding.PING_ENTRY_DTYPE, "pirip_spec_band_row": binding.SPEC_BAND_ROW_DTYPE}


def _structs():
    """name -> [field names] of every `typedef struct TAG { ... } NAME;` of the header"""
    out = {}
    for tag, body, name in re.findall(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;", _header(), flags=re.S):
        fields = []
        for decl in filter(None, (" ".join(d.split()) for d in body.split(";"))):
            first, *more = decl.split(",")
            for declarator in [first.rsplit(" ", 1)[1]] + more:
                fields.append(re.fullmatch(r"\s*\**\s*(\w+)\s*(\[\d+\])?\s*", declarator).group(1))
        out[name] = fields
    return out


@pytest.fixture(scope="module")
def c_layouts(tmp_path_factory):
    """name -> (sizeof, [(field, offsetof, sizeof field)]) as gcc lays the header's structures out"""
    d = tmp_path_factory.mktemp("layouts")
    lines = ['#include <stdio.h>', '#include "pirip_hip.h"', "int main(void) {"]
    for name, fields in _structs().items():
        lines.append(f'    printf("S {name} %zu\\n", sizeof({name}));')
        lines += [f'    printf("F {name} {f} %zu %zu\\n", offsetof({name}, {f}), sizeof((({name} *)0)->{f}));' for f in fields]
    lines += ["    return 0;", "}"]
    (d / "layouts.c").write_text("\n".join(lines) + "\n")
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(d / "layouts"), str(d / "layouts.c")], check=True)
    out = {}
    for ln in subprocess.run([str(d / "layouts")], check=True, capture_output=True, text=True).stdout.splitlines():
        kind, name, *rest = ln.split()
        if kind == "S":
            out[name] = (int(rest[0]), [])
        else:
            out[name][1].append((rest[0], int(rest[1]), int(rest[2])))
    return out


def test_every_structure_of_the_header_has_a_twin(c_layouts):
    assert len(c_layouts) >= 22 and set(c_layouts) == set(_structs())
    assert set(c_layouts) == set(TWINS) | set(DTYPES), sorted(set(c_layouts) ^ (set(TWINS) | set(DTYPES)))
    assert c_layouts["pirip_stream_state"][0] == 52                          # 13 words, not 14


@pytest.mark.parametrize("name", sorted(TWINS))
def test_ctypes_structure_has_the_c_layout(c_layouts, name):
    size, fields = c_layouts[name]
    T = TWINS[name]
    assert C.sizeof(T) == size, (name, C.sizeof(T), size)
    assert [(n, getattr(T, n).offset, getattr(T, n).size) for n, *_ in T._fields_] == fields, name


@pytest.mark.parametrize("name", sorted(DTYPES))
def test_numpy_dtype_has_the_c_layout(c_layouts, name):
    size, fields = c_layouts[name]
    dt = np.dtype(DTYPES[name])
    assert dt.itemsize == size
    assert [(n, dt.fields[n][1], dt.fields[n][0].itemsize) for n in dt.names] == fields, name


# ---------------------------------------------------------------- the public surface

def public_api(mod):
    def sig(o):
        try:
            return str(inspect.signature(o))
        except (TypeError, ValueError):
            return None
    names = sorted(n for n in vars(mod) if not n.startswith("_") and not inspect.ismodule(getattr(mod, n)))
    sigs = {}
    for n in names:
        o = getattr(mod, n)
        if inspect.isclass(o):
            sigs[n] = sig(o)
            sigs.update({f"{n}.{m}": sig(f) for m, f in inspect.getmembers(o, inspect.isfunction) if not m.startswith("_")})
        elif inspect.isfunction(o):
            sigs[n] = sig(o)
    return {"names": names, "signatures": sigs}


def test_the_public_surface_only_grows():
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "binding_api.json")))
    got = public_api(pirip_amd)
    assert len(want["names"]) >= 52 and len(want["signatures"]) >= 137
    assert not set(want["names"]) - set(got["names"]), sorted(set(want["names"]) - set(got["names"]))
    changed = {k: (v, got["signatures"].get(k)) for k, v in want["signatures"].items() if got["signatures"].get(k, "missing") != v}
    assert not changed, changed
