#!/usr/bin/env python
"""Static instruction counts of the convolution kernels by phase: before the first MFMA, the main loop, after the last MFMA.

Compiles csrc/dt_conv_strip.hip, dt_conv_bf16.hip and dt_conv.hip device-only to gfx950 assembly (``hipcc -O3 -S``) and
prints one line per convolution kernel:

    total   instructions of the kernel
    pre     instructions before the first MFMA (argument loads, row and mask arithmetic, the first staging)
    post    instructions after the last MFMA (the staged epilogue in all its modes)
    loop    instructions of the main loop -- the backward branch whose span holds the most MFMAs, the shortest such span
    loopM   MFMAs inside it
    mfma    MFMAs in the kernel
    div     integer-division expansions (counted as v_rcp_iflag_f32), and those after the last MFMA
    VGPR    allocated vector registers;  spill = spilled VGPRs;  scratch = bytes per lane

These are counts of instructions in the code, not of executed ones (the epilogue's modes are run-time flags; executed
counts come from the SQ counters, tools/conv_fixed_counters.py).  Nothing is run; no GPU is needed.

    python tools/kernel_phases.py                   # the three sources
    python tools/kernel_phases.py dt_conv_strip.hip
"""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from distillation_trajectories_amd.csrc import build as _build  # noqa: E402
from kernel_resources import short_name  # noqa: E402

SOURCES = ["dt_conv_strip.hip", "dt_conv_bf16.hip", "dt_conv.hip"]
KERNELS = re.compile(r"^(conv_strip_bf16x6_kernel|conv_gemm_bf16x6_kernel|conv_gemm_kernel|splitk_epilogue_kernel)<")
FIELDS = ("total", "pre", "post", "loop", "loop_mfma", "mfma", "div", "div_post", "vgprs", "spill", "scratch")
_LABEL = re.compile(r"^([.\w$]+):")
_INSTR = re.compile(r"^\s+([a-z][a-z0-9_]*)\b(.*)$")
_BRANCH = re.compile(r"^s_c?branch")


def assembly(source):
    path = source if os.path.isabs(source) else os.path.join(_build.HERE, source)
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "out.s")
        cmd = [_build.hipcc_path(), f"--offload-arch={_build.ARCH}", "-O3", "-std=c++17", "--cuda-device-only", "-S", path, "-o", out]
        res = subprocess.run(cmd, capture_output=True, text=True)
        if res.returncode != 0:
            raise RuntimeError(f"hipcc failed on {path}:\n{res.stderr}")
        with open(out) as f:
            return f.read()


def _metadata(text):
    """{symbol: {vgprs, spill, scratch}} from the code object's metadata notes"""
    out, cur = {}, None
    for line in text.splitlines():
        if re.match(r"^  - \.", line):
            cur = {}
        m = re.match(r"^\s+(?:- )?\.(name|vgpr_count|vgpr_spill_count|private_segment_fixed_size):\s*(\S+)", line)
        if cur is not None and m:
            cur[m.group(1)] = m.group(2)
            if "name" in cur:
                out[cur["name"]] = cur
    return {k: {"vgprs": int(v.get("vgpr_count", -1)), "spill": int(v.get("vgpr_spill_count", -1)),
                "scratch": int(v.get("private_segment_fixed_size", -1))} for k, v in out.items()}


def kernel_phases(text):
    """{kernel name: counts} of every convolution kernel in one assembly listing"""
    meta, out = _metadata(text), {}
    lines = text.splitlines()
    i = 0
    while i < len(lines):
        m = _LABEL.match(lines[i])
        if not (m and m.group(1).startswith("_Z") and KERNELS.match(short_name(m.group(1)))):
            i += 1
            continue
        sym, ops, labels = m.group(1), [], {}
        i += 1
        while i < len(lines) and not lines[i].startswith(".Lfunc_end"):
            lab = _LABEL.match(lines[i])
            if lab:
                labels[lab.group(1)] = len(ops)
            else:
                ins = _INSTR.match(lines[i].split(";")[0])
                if ins:
                    ops.append((ins.group(1), ins.group(2)))
            i += 1
        mf = [k for k, (op, _) in enumerate(ops) if op.startswith("v_mfma")]
        div = [k for k, (op, _) in enumerate(ops) if op.startswith("v_rcp_iflag_f32")]
        c = {"total": len(ops), "mfma": len(mf), "div": len(div), "pre": mf[0] if mf else len(ops),
             "post": len(ops) - 1 - mf[-1] if mf else 0, "div_post": len([k for k in div if mf and k > mf[-1]]),
             "loop": 0, "loop_mfma": 0}
        for k, (op, arg) in enumerate(ops):
            if not _BRANCH.match(op):
                continue
            start = labels.get(arg.strip())
            if start is None or start > k:
                continue
            n = len([j for j in mf if start <= j <= k])
            if n > c["loop_mfma"] or (n == c["loop_mfma"] and n and k + 1 - start < c["loop"]):
                c["loop"], c["loop_mfma"] = k + 1 - start, n
        c.update(meta.get(sym, {"vgprs": -1, "spill": -1, "scratch": -1}))
        out[short_name(sym)] = c
    return out


def report(sources=None):
    """[(source, {kernel: counts})] of the convolution sources"""
    sources = sources or SOURCES
    with ThreadPoolExecutor(max_workers=len(sources)) as pool:
        texts = list(pool.map(assembly, sources))
    return [(os.path.basename(s), kernel_phases(t)) for s, t in zip(sources, texts)]


def format_report(rep):
    head = f"{'kernel':<44} {'total':>6} {'pre':>6} {'post':>6} {'loop':>6} {'loopM':>6} {'mfma':>5} {'div':>4} {'divpost':>7} {'VGPR':>5} {'spill':>6} {'scratch':>8}"
    rows = [head]
    for src, kernels in rep:
        rows.append(f"# {src}")
        for name, c in sorted(kernels.items()):
            rows.append(f"{name:<44} {c['total']:>6} {c['pre']:>6} {c['post']:>6} {c['loop']:>6} {c['loop_mfma']:>6} {c['mfma']:>5} "
                        f"{c['div']:>4} {c['div_post']:>7} {c['vgprs']:>5} {c['spill']:>6} {c['scratch']:>8}")
    return "\n".join(rows) + "\n"


def parse_report(text):
    """{kernel: counts} of a committed report (the inverse of format_report).  The reports from before the strip kernel had
    its NH parameter name it <BM,BN,KC,WK>: those are today's <BM,BN,KC,WK,1>."""
    out = {}
    for line in text.splitlines():
        parts = line.split()
        if len(parts) == 1 + len(FIELDS) and KERNELS.match(parts[0]):
            name = re.sub(r"^(conv_strip_bf16x6_kernel<\d+,\d+,\d+,\d+)>$", r"\1,1>", parts[0])
            out[name] = dict(zip(FIELDS, (int(v) for v in parts[1:])))
    return out


def main(argv):
    sys.stdout.write(format_report(report(argv or None)))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
