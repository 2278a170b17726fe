"""The ctypes prototypes of the thirteen add-on bindings against tests/golden/binding_prototypes.json, which
tools/dump_binding_prototypes.py wrote from the bindings as they stood before they were given a shared layer: every name in a
module's SYMBOLS has exactly the recorded restype and argtypes, and the record names nothing else. A binding that sets a
prototype from a table instead of statement by statement cannot drop or change one unnoticed. Host only."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import dump_binding_prototypes as dump  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as g

    g.build()


@pytest.fixture(scope="module")
def recorded(golden_dir):
    with open(os.path.join(golden_dir, "binding_prototypes.json")) as f:
        return json.load(f)


def test_the_record_covers_the_thirteen_libraries(recorded):
    assert set(recorded) == set(dump.MODULES)
    assert len(dump.MODULES) == 13


@pytest.mark.parametrize("name", dump.MODULES)
def test_every_symbol_has_the_recorded_prototype(recorded, name):
    import importlib

    import tensor_fft_amd  # noqa: F401

    mod = importlib.import_module("tensor_fft_amd." + name)
    assert set(recorded[name]) == set(mod.SYMBOLS), set(recorded[name]) ^ set(mod.SYMBOLS)
    assert len(mod.SYMBOLS) == len(set(mod.SYMBOLS))
    if hasattr(mod, "_prototypes"):           # a module that sets its prototypes from a table of its own: the table names nothing else
        assert set(mod._prototypes()) == set(mod.SYMBOLS), set(mod._prototypes()) ^ set(mod.SYMBOLS)
    lib = getattr(mod, f"load_{name}_library")()
    for sym in mod.SYMBOLS:
        got = dump.prototype(getattr(lib, sym))
        assert got == recorded[name][sym], (sym, got, recorded[name][sym])
        assert got[1] is not None, f"{sym}: argtypes never set"
