#!/usr/bin/env python3
"""The cheapest cell of every plan the selection ladder can print (host only -- needs no GPU): a fixed lattice of (M, N, K, registered weight
image) goes through mixq_describe_plan with every knob at its default, the cells are grouped by the text they get, and per text the cell with
the smallest M*N*K + N*K is kept.  Writes tests/golden/plan_cells.json:

  "cells"    {plan, M, N, K, image}: one per plan text whose cheapest cell has M*N*K <= 120e9 -- tests/test_gpu_plan_cells.py runs each of them
             through mixq_enqueue and checks every output element;
  "named"    the same records + "name" and "reason": cells chosen by hand for plan attributes the text does not show;
  "not_run"  {plan, M, N, K, image, cost}: texts the lattice reaches only above that cost, listed instead of dropped.

tests/test_abi.py::test_plan_cells_are_the_pinned_ones pins the file and asserts that every text of tests/golden/selection_table.json has a cell.
usage: python tools/plan_cells.py [--check]"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mixq_tensorrt_llm_amd import _lib  # noqa: E402

# the ladder's edges in M (4 | 5, 16 | 17, 32 | 33, 48 | 49, 64 | 65, 96 | 97, 128 | 129, 256 | 257, tile-row counts of the 128- and 256-row tiles)
ROWS = [1, 4, 5, 16, 17, 32, 33, 48, 49, 64, 65, 96, 97, 128, 129, 160, 193, 256, 257, 320, 385, 512, 513, 768, 1025, 1536, 2048, 2049, 4096,
        8192, 16384, 65536]
# N: the BASELINE widths and powers of two around them; 272, 5136 and 12304 are 16 past a multiple of 128 (a last tile of 16 columns)
COLS = [256, 272, 1024, 1280, 2048, 3072, 3584, 4096, 4608, 5136, 6144, 8192, 8960, 11008, 12288, 12304, 16384, 18944, 24576, 28672, 32768]
# K: 1088 and 4160 are 64 past a multiple of 128 (half a last slice), 3200 and 8320 128 past a multiple of 256 (whole slices, no 256-byte runs)
DEPTHS = [1024, 1088, 2048, 3072, 3200, 3584, 4096, 4160, 5120, 8192, 8320, 11008, 16384, 25600, 28672]
MAX_MNK = 120 * 10 ** 9

NAMED = [
    ("mid-rotated-walk", 513, 4096, 3072, 0, "mid kernel, 5 tile rows, K not split: the rotated K walk applies by rule (knob 1411 switches it off)"),
    ("skinny-runs-nontemporal", 5, 8192, 4096, 0, "256-byte-run route on a 32 MiB weight: the loads are non-temporal by rule (knob 887 switches that off)"),
    ("tiles-nontemporal", 49, 12288, 4096, 0, "one tile row of 64x64 tiles on a 48 MiB weight: non-temporal weight copies by rule (knob 1291 switches them off)"),
    ("mid-96-scratch", 641, 880, 8192, 0, "mid kernel, 96-wide tiles, 4 workgroups per tile along K: 60 parked tiles of 128x96 need more scratch than the 42 tiles of 128x128 (gemm_deep_workspace_size takes the larger)"),
    ("decode-small", 4, 256, 1024, 0, "M <= 4: one launch on qweight"),
    ("decode-small-neighbour", 5, 256, 1024, 0, "the M = 5 neighbour of decode-small: quantiser + skinny GEMM on the int8 weight"),
    ("decode-large-neighbour", 4, 8192, 4096, 0, "the M = 4 neighbour of skinny-runs-nontemporal: one launch on a 32 MiB qweight"),
]


def cost(M, N, K):
    return M * N * K + N * K


def describe(lib, buf, M, N, K, image):
    assert lib.mixq_describe_plan(M, N, K, image, buf, 320) == 0
    return buf.value.decode()


def cells():
    lib = _lib.load()
    lib.mixq_debug_reset()
    buf = ctypes.create_string_buffer(320)
    best = {}
    for M in ROWS:
        for N in COLS:
            for K in DEPTHS:
                for image in (0, 1):
                    plan = describe(lib, buf, M, N, K, image)
                    key = (cost(M, N, K), M, N, K, image)
                    if plan not in best or key < best[plan]:
                        best[plan] = key
    run, not_run = [], []
    for plan, (c, M, N, K, image) in sorted(best.items(), key=lambda kv: kv[1]):
        rec = {"plan": plan, "M": M, "N": N, "K": K, "image": image}
        if M * N * K <= MAX_MNK:
            run.append(rec)
        else:
            not_run.append(dict(rec, cost=c))
    named = [{"name": name, "plan": describe(lib, buf, M, N, K, image), "M": M, "N": N, "K": K, "image": image, "reason": why}
             for name, M, N, K, image, why in NAMED]
    return {"lattice": {"M": ROWS, "N": COLS, "K": DEPTHS, "max_MNK": MAX_MNK}, "cells": run, "named": named, "not_run": not_run}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="compare with the pinned file instead of writing it")
    a = ap.parse_args()
    got = cells()
    gold = os.path.join(ROOT, "tests", "golden", "plan_cells.json")
    if a.check:
        want = json.load(open(gold))
        bad = 0
        for part in ("lattice", "cells", "named", "not_run"):
            if got[part] == want.get(part):
                continue
            bad += 1
            print(f"{part} differs from the pinned file:")
            if part == "lattice":
                continue
            key = lambda r: (r.get("name"), r["plan"])  # noqa: E731
            pinned, now = {key(r): r for r in want.get(part, [])}, {key(r): r for r in got[part]}
            for k in sorted(set(pinned) | set(now), key=str):
                if pinned.get(k) != now.get(k):
                    print(f"   pinned {pinned.get(k)!r}\n   library says {now.get(k)!r}")
        print(f"{bad} part(s) differ")
        return 1 if bad else 0
    with open(gold, "w") as f:
        json.dump(got, f, indent=1)
        f.write("\n")
    print(f"wrote {gold}: {len(got['cells'])} cells, {len(got['named'])} named, {len(got['not_run'])} not run")
    return 0


if __name__ == "__main__":
    sys.exit(main())
