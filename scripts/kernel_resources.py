#!/usr/bin/env python3
"""Compile one csrc/*.hip file for gfx950 with -Rpass-analysis=kernel-resource-usage and print one row per kernel:
SGPRs, VGPRs, AGPRs, scratch bytes per lane, static LDS bytes, occupancy.  Needs hipcc, no GPU.

    python scripts/kernel_resources.py constriction_amd/csrc/cst_indexed_ragged.hip [--filter indexed_ragged] [--markdown]

Exits 1 if any listed kernel uses scratch memory."""
import argparse
import re
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from constriction_amd import build  # noqa: E402

FIELDS = (("SGPRs", "sgpr"), ("VGPRs", "vgpr"), ("AGPRs", "agpr"), ("ScratchSize [bytes/lane]", "scratch"), ("Occupancy [waves/SIMD]", "occupancy"),
          ("LDS Size [bytes/block]", "lds"))


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
    return out.stdout.splitlines() if out.returncode == 0 else names


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("source")
    ap.add_argument("--filter", default="", help="only kernels whose demangled name contains this")
    ap.add_argument("--markdown", action="store_true")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        res = subprocess.run([build._hipcc(), *build.FLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", args.source, "-o", str(Path(tmp) / "x.o")],
                             capture_output=True, text=True)
    if res.returncode != 0:
        sys.exit(res.stderr)
    kernels, cur = [], None
    for line in res.stderr.splitlines():
        m = re.search(r"remark: .*Function Name: (\S+)", line)
        if m:
            cur = {"name": m.group(1)}
            kernels.append(cur)
            continue
        for label, key in FIELDS:
            m = re.search(r"remark: .*" + re.escape(label) + r": (\d+)", line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    for k, name in zip(kernels, demangle([k["name"] for k in kernels])):
        k["name"] = re.sub(r"^void cst::", "", name).split("(")[0]
    kernels = [k for k in kernels if args.filter in k["name"]]
    keys = [key for _, key in FIELDS]
    if args.markdown:
        print("| kernel | " + " | ".join(keys) + " |")
        print("|---|" + "---:|" * len(keys))
    for k in kernels:
        cells = [str(k.get(key, "?")) for key in keys]
        print(("| `%s` | " % k["name"] + " | ".join(cells) + " |") if args.markdown else "%-90s %s" % (k["name"], " ".join("%s=%s" % kv for kv in zip(keys, cells))))
    sys.exit(1 if any(k.get("scratch", 0) for k in kernels) else 0)


if __name__ == "__main__":
    main()
