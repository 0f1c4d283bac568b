#!/usr/bin/env python
"""Register and scratch figures of every kernel, as the compiler reports them.

Compiles the library's .hip files device-only for gfx950 with ``-Rpass-analysis=kernel-resource-usage`` and prints one
line per kernel: VGPRs, AGPRs, spilled VGPRs, scratch bytes per lane, occupancy (waves per SIMD) and static LDS.
Nothing is run; no GPU is needed.

    python tools/kernel_resources.py                      # every source of the library
    python tools/kernel_resources.py dt_conv_strip.hip    # one file
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from distillation_trajectories_amd.csrc import build as _build  # noqa: E402

FIELDS = (("VGPRs", "vgprs"), ("AGPRs", "agprs"), ("VGPRs Spill", "vgpr_spill"), ("SGPRs Spill", "sgpr_spill"),
          ("ScratchSize [bytes/lane]", "scratch_bytes"), ("Occupancy [waves/SIMD]", "occupancy"),
          ("LDS Size [bytes/block]", "lds_bytes"))
_REMARK = re.compile(r":\d+:\d+: remark:\s*(.+?):\s*(\S+)\s*\[-Rpass-analysis=kernel-resource-usage\]")


def short_name(sym):
    """'_ZN2dt24conv_strip_bf16x6_kernelILi64ELi64ELi4ELi4EEEvNS_10ConvParamsE' -> 'conv_strip_bf16x6_kernel<64,64,4,4>':
    the nested name without its namespaces, integer and bool template arguments; anything else comes back as it is"""
    m = re.match(r"_ZN?", sym)
    if not m:
        return sym
    pos, parts = m.end(), []
    while True:
        n = re.match(r"(\d+)", sym[pos:])
        if not n:
            break
        pos += n.end()
        parts.append(sym[pos:pos + int(n.group(1))])
        pos += int(n.group(1))
    if not parts:
        return sym
    name = parts[-1]
    if sym[pos:pos + 1] == "I":
        args = re.match(r"I((?:L[a-z]n?\d+E)+)E", sym[pos:])
        if not args:
            return sym
        vals = re.findall(r"L[a-z](n?)(\d+)E", args.group(1))
        name += "<" + ",".join(("-" if neg else "") + v for neg, v in vals) + ">"
    return name


def kernel_resources(source):
    """{kernel name: {vgprs, agprs, vgpr_spill, sgpr_spill, scratch_bytes, occupancy, lds_bytes}} of one .hip file of csrc/."""
    path = source if os.path.isabs(source) else os.path.join(_build.HERE, source)
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [_build.hipcc_path(), f"--offload-arch={_build.ARCH}", "-O3", "-std=c++17", "--cuda-device-only",
               "-Rpass-analysis=kernel-resource-usage", "-c", path, "-o", os.path.join(tmp, "out.o")]
        res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError(f"hipcc failed on {path}:\n{res.stderr}")
    kernels, cur = {}, None
    for line in res.stderr.splitlines():
        m = _REMARK.search(line)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2)
        if key == "Function Name":
            cur = kernels.setdefault(val, {})
        elif cur is not None:
            for label, field in FIELDS:
                if key == label:
                    cur[field] = int(val)
    return {short_name(k): v for k, v in kernels.items()}


def strip_template_args(name):
    """(BM, BN, KC, WK) of a conv_strip_bf16x6_kernel<BM,BN,KC,WK[,NH]> name, None for any other kernel"""
    m = re.match(r"conv_strip_bf16x6_kernel<([\d,]+)>$", name)
    return tuple(int(v) for v in m.group(1).split(","))[:4] if m else None


def main(argv):
    sources = argv or _build.SOURCES
    print(f"{'kernel':<58} {'VGPR':>5} {'AGPR':>5} {'spill':>6} {'scratch B':>10} {'occ':>4} {'LDS B':>7}")
    for src in sources:
        print(f"# {os.path.basename(src)}")
        for name, r in sorted(kernel_resources(src).items()):
            print(f"{name:<58} {r.get('vgprs', -1):>5} {r.get('agprs', -1):>5} {r.get('vgpr_spill', -1):>6} "
                  f"{r.get('scratch_bytes', -1):>10} {r.get('occupancy', -1):>4} {r.get('lds_bytes', -1):>7}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
