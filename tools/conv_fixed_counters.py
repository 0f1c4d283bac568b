#!/usr/bin/env python
"""Executed instructions per wave of every convolution kernel, from rocprofv3 counter runs of the benchmark.

Reads the `*_counter_collection.csv` files of one or more `rocprofv3 --pmc ...` runs (each run its own process, no tracing
in it) and, optionally, the `*_kernel_stats.csv` of a separate `--kernel-trace --stats` run, and prints one JSON document:
per kernel name the launches, the waves, each SQ_INSTS_* counter summed over the launches, and per wave and launch the
executed VALU (MFMA excluded), SALU, MFMA, LDS, VMEM-read and SMEM instructions and their non-MFMA sum.  No GPU is needed.

    python tools/conv_fixed_counters.py --stats t_kernel_stats.csv p1_counter_collection.csv p2_counter_collection.csv
"""
import argparse
import csv
import json
import re
import sys
from collections import defaultdict

CONV = re.compile(r"conv_strip_bf16x6_kernel|conv_gemm_bf16x6_kernel|conv_gemm_kernel|splitk_epilogue_kernel")


def short(name):
    return re.sub(r"^void dt::|\(dt::ConvParams\)$|\s", "", name)


def read_counters(paths):
    """{kernel: {counter: sum}}, {kernel: launches}; a counter present in several runs (SQ_WAVES) is taken from the first"""
    sums, launches, owner = defaultdict(lambda: defaultdict(float)), defaultdict(set), {}
    for path in paths:
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                name = row["Kernel_Name"]
                if not CONV.search(name):
                    continue
                k, c = short(name), row["Counter_Name"]
                if owner.setdefault(c, path) != path:
                    continue
                sums[k][c] += float(row["Counter_Value"])
                launches[k].add((path, row["Dispatch_Id"]))
    first = paths[0] if paths else None
    return sums, {k: len([1 for p, _ in v if p == first]) for k, v in launches.items()}


def read_stats(path):
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            if CONV.search(row["Name"]):
                out[short(row["Name"])] = {"calls": int(row["Calls"]), "average_us": float(row["AverageNs"]) / 1e3,
                                           "total_ms": float(row["TotalDurationNs"]) / 1e6}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stats", default=None, help="kernel_stats.csv of a separate kernel-trace run")
    ap.add_argument("--note", default="")
    ap.add_argument("counters", nargs="*")
    args = ap.parse_args()
    sums, launches = read_counters(args.counters)
    stats = read_stats(args.stats) if args.stats else {}
    doc = {"note": args.note, "kernels": {}}
    for k in sorted(set(sums) | set(stats)):
        c = dict(sums.get(k, {}))
        e = {"trace": stats.get(k), "counter_run_launches": launches.get(k, 0), "counters": c}
        waves = c.get("SQ_WAVES", 0.0)
        if waves:
            per = {n: c.get("SQ_INSTS_" + n, 0.0) / waves for n in ("VALU", "MFMA", "SALU", "LDS", "VMEM_RD", "SMEM")}
            per["VALU_without_MFMA"] = per["VALU"] - per["MFMA"]
            per["non_MFMA"] = per["VALU_without_MFMA"] + per["SALU"] + per["LDS"] + per["VMEM_RD"] + per["SMEM"]
            e["waves_per_launch"] = waves / max(1, launches.get(k, 1))
            e["per_wave"] = {n: round(v, 1) for n, v in per.items()}
        doc["kernels"][k] = e
    json.dump(doc, sys.stdout, indent=1)
    print()
    return 0


if __name__ == "__main__":
    sys.exit(main())
