#!/usr/bin/env python3
"""The ctypes prototypes the thirteen add-on bindings set, by type name (tests/golden/binding_prototypes.json).

    python tools/dump_binding_prototypes.py [--out FILE]

For every add-on module (nine convolution, four STFT) the library is loaded through the module's own load_*_library, and every name
in its SYMBOLS is recorded as [restype, [argtypes...]]: "c_uint64", "POINTER(GconvOpts)", null for a void result, and null in place
of the list for a function whose argtypes were never set. tests/test_binding_prototypes_host.py holds the bindings to the file,
so it is written once, from the commit a change of the binding layer starts from, and not again. Host only, no GPU needed."""
import argparse
import ctypes
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODULES = ("conv", "lconv", "sconv", "gconv", "gsconv", "bconv", "gbconv", "cconv", "gcconv", "stft", "istft", "stftn", "istftn")
# ctypes aliases the fixed-width and the C names (c_uint64 is c_ulong here, and so is c_size_t): a type goes by the first name in
# this list that is the same object, so the file does not depend on which of its names a binding wrote
_NAMES = ("c_void_p", "c_char_p", "c_int", "c_uint32", "c_uint64", "c_int32", "c_int64", "c_size_t", "c_float", "c_double")


def type_name(t):
    if t is None:
        return None
    for name in _NAMES:
        if t is getattr(ctypes, name):
            return name
    if hasattr(t, "_type_") and not isinstance(t._type_, str):       # POINTER(X)
        return f"POINTER({type_name(t._type_)})"
    return t.__name__                                                # a Structure


def prototype(fn):
    return [type_name(fn.restype), None if fn.argtypes is None else [type_name(a) for a in fn.argtypes]]


def module_table(name):
    """{symbol: [restype, [argtypes...]]} of tensor_fft_amd.<name>, over its SYMBOLS"""
    import tensor_fft_amd  # noqa: F401

    mod = importlib.import_module("tensor_fft_amd." + name)
    lib = getattr(mod, f"load_{name}_library")()
    return {sym: prototype(getattr(lib, sym)) for sym in mod.SYMBOLS}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "binding_prototypes.json"))
    args = ap.parse_args()
    import __graft_entry__ as g

    g.build()
    table = {name: module_table(name) for name in MODULES}
    with open(args.out, "w") as f:
        libs = []                   # one line per symbol
        for name in sorted(table):
            rows = ",\n".join(f"  {json.dumps(sym)}: {json.dumps(proto)}" for sym, proto in sorted(table[name].items()))
            libs.append(f" {json.dumps(name)}: {{\n{rows}\n }}")
        f.write("{\n" + ",\n".join(libs) + "\n}\n")
    print(f"{args.out}: {sum(len(t) for t in table.values())} symbols of {len(table)} libraries")


if __name__ == "__main__":
    main()
