#!/usr/bin/env python3
"""Records tests/golden/mixlib_refusals.json: what every call of the grid in tests/test_mixlib_refusal_table.py is answered with -- the
exception's class and text, or "returned" -- when the mixlib ops (and mixlinear.find_outliers / dequant_weight_columns) get CPU tensors.

    python tools/record_mixlib_refusals.py [--out tests/golden/mixlib_refusals.json]

Run it on the tree whose answers are the accepted ones (the commit a refactor of the wrappers starts from): the table then pins the
class, the text and so the order of every Python-side check.  No device is needed or touched.  The file holds each distinct outcome
once and one index per call, per op in the grid's order, with a digest of that op's case ids."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "mixlib_refusals.json"))
    args = ap.parse_args()
    import test_mixlib_refusal_table as T
    seen, ops = [], {}
    for op, cases in T.by_op().items():
        index = []
        for _, fn in cases:
            o = T.outcome(fn)
            if o not in seen:
                seen.append(o)
            index.append(seen.index(o))
        ops[op] = {"ids": T.ids_digest(cases), "index": index}
    with open(args.out, "w") as f:
        f.write('{"count": %d,\n"outcomes": [\n' % len(T.CASES))
        f.write(",\n".join(json.dumps(o) for o in seen))
        f.write('\n],\n"ops": {\n')
        f.write(",\n".join(f"{json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in ops.items()))
        f.write("\n}}\n")
    print(f"{len(T.CASES)} calls of {len(ops)} ops, {len(seen)} distinct outcomes -> {args.out}")


if __name__ == "__main__":
    main()
