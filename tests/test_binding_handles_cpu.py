"""The life cycle every handle class of pirip_amd/binding.py inherits from its one base class, against a stub in the place of the loaded
library (binding._lib, the seam lib() reads): no device, no library. The stub knows the entry points of binding.SIGNATURES only, checks
each call's arity against the table, records (name, args) and returns a chosen status.

  * a created handle is destroyed exactly once, however often it is closed, and h is None afterwards;
  * a create that fails (PIRIP_ERR_NO_DEVICE) raises PiripError and leaves nothing to destroy: close() and the object's end make no call;
  * a method of a closed handle raises PiripError before any C call: C never sees a NULL handle from here;
  * __del__ swallows whatever close() raises.
tests/test_binding_lifecycle.py walks the same classes and the same methods on the device."""
import gc

import pytest

import pirip_amd
from pirip_amd import binding

ERR_NO_DEVICE = -3


class StubLib:
    def __init__(self, fail=()):
        self.calls, self.fail = [], set(fail)

    def __getattr__(self, name):
        if name not in binding.SIGNATURES:
            raise AttributeError(name)

        def fn(*args):
            assert len(args) == len(binding.SIGNATURES[name][1]), (name, args)
            self.calls.append((name, args))
            if name == "pirip_hip_strerror":
                return b"stub"
            if name in self.fail:
                return ERR_NO_DEVICE
            if "create" in name:
                args[-1]._obj.value = 0x1000 + len(self.calls)          # the handle out: byref of a c_void_p
            return 0
        return fn

    def named(self, name):
        return [c for c in self.calls if c[0] == name]


def _tx_side(b):
    tx = b.HipTx("no.code", 40000, 1000, 2)
    return tx, b.HipTxStream(tx, b.HipMux(240000, 6, [0]), 24000, 1000)


def _rx(b):
    return b.HipRx(b.HipDemod(40000, 1000, 2, P=10, in_format=b.IN_CF32), ldpc=b.HipLdpc("no.code", 2), chan=b.HipChan(240000, 6, [0]), block=24000)


# class name -> (its create entry points, a function of the module that returns the constructor's arguments: the handles it needs are
# built in there, and (method name, arguments) of one call that must raise once the handle is closed)
CASES = {
    "HipDemod": (["pirip_hip_create", "pirip_hip_create_recalled"], lambda b: ((240000, 10000, 2), {}), ("reset", ())),
    "HipDecim": (["pirip_hip_decim_create"], lambda b: ((45,), {}), ("taps", ())),
    "HipLdpc": (["pirip_hip_ldpc_create"], lambda b: (("no.code", 2), {}), ("reset", ())),
    "HipChan": (["pirip_hip_chan_create"], lambda b: ((240000, 6, [0]), {}), ("nout", (1000,))),
    "HipMux": (["pirip_hip_mux_create"], lambda b: ((240000, 6, [0]), {}), ("taps", ())),
    "HipTx": (["pirip_hip_tx_create"], lambda b: (("no.code", 40000, 1000, 2), {}), ("max_syms", (1,))),
    "HipTxStream": (["pirip_hip_txs_create"], lambda b: ((b.HipTx("no.code", 40000, 1000, 2), b.HipMux(240000, 6, [0]), 24000, 1000), {}),
                    ("reset", ())),
    "HipRx": (["pirip_hip_rx_create", "pirip_hip_rx_create_chan"],
              lambda b: ((b.HipDemod(40000, 1000, 2, P=10, in_format=b.IN_CF32),), dict(dec=b.HipDecim(6, out_s16=False), block=18000)),
              ("input", ())),
    "HipTestBits": (["pirip_hip_tbits_create"], lambda b: ((), {}), ("counters", ())),
    "HipRepeater": (["pirip_hip_rpt_create"], lambda b: (_tx_side(b) + ([0], 2), dict(rx=_rx(b))), ("offered", ())),
    "HipPing": (["pirip_hip_ping_create"], lambda b: ((_rx(b),) + _tx_side(b), {}), ("records", ())),
    "HipAir": (["pirip_hip_air_create", "pirip_hip_air_create_ex", "pirip_hip_air_create_fade"],
               lambda b: ((240000, [(0, 0, 1.0, 0, 0)], 1, 1), {}), ("drift", ())),
    "HipSpectrum": (["pirip_hip_spec_create"], lambda b: ((240000, 256), {}), ("band_bins", (0,))),
}


def test_every_handle_class_is_covered():
    handles = {n for n, c in vars(binding).items() if isinstance(c, type) and issubclass(c, binding._Handle) and not n.startswith("_")}
    assert handles == set(CASES) and len(handles) == 13
    assert all(getattr(pirip_amd, n) is getattr(binding, n) for n in CASES)
    # close and __del__ are written once, in the base class
    assert all("close" not in vars(getattr(binding, n)) and "__del__" not in vars(getattr(binding, n)) for n in CASES)
    assert "close" not in vars(binding._Terminal) and "__del__" not in vars(binding._Terminal)


def _stubbed(monkeypatch, fail=()):
    stub = StubLib(fail)
    monkeypatch.setattr(binding, "_lib", stub)
    assert binding.lib() is stub
    return stub


@pytest.mark.parametrize("name", sorted(CASES))
def test_destroy_runs_once_and_a_closed_handle_raises_before_c(monkeypatch, name):
    stub = _stubbed(monkeypatch)
    creates, make, (method, margs) = CASES[name]
    cls = getattr(binding, name)
    args, kw = make(binding)
    h = cls(*args, **kw)
    assert h.L is stub and h.h is not None and len([c for c in stub.calls if c[0] in creates]) == 1
    if cls._Info is not None:                                  # the create helper read the info structure, through the handle
        assert isinstance(h.info, cls._Info) and [c[1][0] for c in stub.named(cls._c + "_get_info")][-1] is h.h
    handle = h.h
    destroy = cls._c + "_destroy"
    before = len(stub.named(destroy))                          # (none: the handles it needs are other classes')
    h.close()
    h.close()
    assert h.h is None
    assert stub.named(destroy)[before:] == [(destroy, (handle,))]
    n = len(stub.calls)
    with pytest.raises(pirip_amd.PiripError, match="closed"):
        getattr(h, method)(*margs)
    assert len(stub.calls) == n, stub.calls[n:]
    del h
    gc.collect()
    assert len(stub.named(destroy)) == before + 1


@pytest.mark.parametrize("name", sorted(CASES))
def test_a_failed_create_leaves_nothing_to_destroy(monkeypatch, name):
    creates, make, _ = CASES[name]
    stub = _stubbed(monkeypatch, fail=creates)
    cls = getattr(binding, name)
    args, kw = make(binding)                                   # (the handles it needs are other classes': their creates succeed)
    h = cls.__new__(cls)
    with pytest.raises(pirip_amd.PiripError, match=r"\(-3\)"):
        h.__init__(*args, **kw)
    assert h.h is None
    n = len(stub.calls)
    h.close()
    del h
    gc.collect()
    assert stub.calls[n:] == [] and not stub.named(cls._c + "_destroy")


def test_the_parents_of_a_handle_must_be_open(monkeypatch):
    stub = _stubbed(monkeypatch)
    tx, mux = binding.HipTx("no.code", 40000, 1000, 2), binding.HipMux(240000, 6, [0])
    tx.close()
    n = len(stub.calls)
    with pytest.raises(pirip_amd.PiripError, match="closed"):
        binding.HipTxStream(tx, mux, 24000, 1000)
    dem, ld = binding.HipDemod(240000, 10000, 2), binding.HipLdpc("no.code", 2)
    dem.close()
    m = len(stub.calls)
    with pytest.raises(pirip_amd.PiripError, match="closed"):
        ld.chain_batch(dem, 0, 0, 0, 0, 0, 0, 0, 0, 1)
    with pytest.raises(pirip_amd.PiripError, match="closed"):
        binding.HipLdpc.chain_batch_groups([(ld, dem, 0, 0, 0, 0, 0, 0)], 0, 0, 1)
    assert len(stub.calls) == m and not [c for c in stub.calls[n:] if "txs" in c[0]]


def test_del_never_raises(monkeypatch):
    _stubbed(monkeypatch)
    h = binding.HipDecim(45)

    class Gone:
        def __getattr__(self, name):
            raise RuntimeError("the library is gone")
    h.L = Gone()
    with pytest.raises(RuntimeError):
        h.close()                                              # close() itself reports it ...
    h.h = 1
    h.__del__()                                                # ... the object's end does not
    assert h.h is None


def test_the_measured_calls_marshal_what_they_were_given(monkeypatch):
    """one C call per Python call on the measured paths, the handle first and the arguments in the header's order"""
    stub = _stubbed(monkeypatch)
    dem, ld = binding.HipDemod(240000, 10000, 2), binding.HipLdpc("no.code", 2)
    rx = binding.HipRx(dem, block=4800)
    n = len(stub.calls)
    dem.demod_batch(11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23)
    ld.chain_batch(dem, 31, 32, 33, 34, 35, 36, 37, 38, 39, 40, 41, 42)
    rx.process(51, 52, 53, 54, 55, 56, 57, 58, 59, 60, 61)
    rx.push(71, 72, 73, 74, 75, 76, 77, 78, 79, 80, 81, 82, 83)
    assert stub.calls[n:] == [
        ("pirip_hip_demod_batch", (dem.h,) + tuple(range(11, 24))),
        ("pirip_hip_fsk_ldpc_rx_batch", (dem.h, ld.h, 31, 32, 33, 34, 35, 36, 40, 41, 37, 38, 39, 42)),
        ("pirip_hip_rx_process", (rx.h,) + tuple(range(51, 62))),
        ("pirip_hip_rx_push", (rx.h,) + tuple(range(71, 84))),
    ]
