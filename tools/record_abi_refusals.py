#!/usr/bin/env python3
"""Records tests/golden/abi_refusals.json: the return code of every call of the grid in tests/test_abi_refusal_table.py, one digit per call.

    python tools/record_abi_refusals.py [--lib path/to/libmixq_mi355x.so] [--out tests/golden/abi_refusals.json]

Run it on a machine WITHOUT a device, against a library whose codes are the accepted ones (a build of the commit a refactor starts
from): the table then pins them.  It aborts on a call that is answered with MIXQ_E_HIP, or with MIXQ_OK while every count is positive --
such a call reached the device, and its code says nothing about the argument checks."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from mixq_tensorrt_llm_amd import _lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib", default=_lib.LIB_PATH)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "abi_refusals.json"))
    args = ap.parse_args()
    import test_abi_refusal_table as T
    if T._has_device():
        raise SystemExit("a device is visible: the grid's dummy pointers must never reach one")
    lib = ctypes.CDLL(args.lib)
    for name, (res, argtypes) in _lib.SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, argtypes
    entries = {e.name: T.codes(lib, e, recording=True) for e in T.ENTRIES}
    with open(args.out, "w") as f:
        f.write('{"abi": %d, "entries": {\n' % lib.mixq_abi_version())
        f.write(",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in entries.items()))
        f.write("\n}}\n")
    print(f"{sum(map(len, entries.values()))} calls of {len(entries)} entries -> {args.out}")


if __name__ == "__main__":
    main()
