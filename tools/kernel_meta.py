"""The code-object metadata of every kernel of a libhalda.so build, as JSON: per kernel the AGPRs, VGPRs,
SGPRs, scratch bytes per lane, spill counts, static LDS, kernarg size and workgroup size that the compiler
wrote into the gfx950 code object (read with the ROCm LLVM tools, as tests/test_abi.py reads them).

    python tools/kernel_meta.py distilp_amd/libhalda.so                      # this build
    python tools/kernel_meta.py NEW.so --against OLD.so --out profiles/kernel_meta.json

With --against, the output holds both builds and the list of kernels whose metadata differs or that only one
build has; DESIGN.md cites it where it says the existing kernels are unchanged.
"""

from __future__ import annotations

import argparse
import json
import re
import subprocess
import sys
import tempfile
from pathlib import Path

LLVM = Path("/opt/rocm/lib/llvm/bin")
KEYS = ("agpr_count", "vgpr_count", "sgpr_count", "private_segment_fixed_size", "vgpr_spill_count",
        "sgpr_spill_count", "group_segment_fixed_size", "kernarg_segment_size", "max_flat_workgroup_size")


def kernel_meta(lib: str) -> dict:
    with tempfile.TemporaryDirectory() as t:
        t = Path(t)
        fat, co = t / "fatbin.bin", t / "gfx950.co"
        subprocess.run([str(LLVM / "llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", lib, str(t / "host.so")],
                       check=True, capture_output=True)
        subprocess.run([str(LLVM / "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={fat}",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True, capture_output=True)
        notes = subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(co)], check=True, capture_output=True,
                               text=True).stdout
    out = {}
    for item in re.split(r"(?m)^  - \.agpr_count:", notes)[1:]:
        kv = dict(re.findall(r"(?m)^    \.(\w+):\s+(\S+)", item))
        kv["agpr_count"] = item.split("\n")[0].strip()
        out[re.search(r"halda_\w+?_kernel", kv["name"]).group(0)] = {k: int(kv[k]) for k in KEYS}
    return dict(sorted(out.items()))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("lib")
    ap.add_argument("--against", help="an older build to compare with")
    ap.add_argument("--out", help="also write the JSON to this file")
    args = ap.parse_args()
    new = kernel_meta(args.lib)
    res = {"kernels": new}
    if args.against:
        old = kernel_meta(args.against)
        res = {"this_build": new, "parent_build": old,
               "only_in_this_build": sorted(set(new) - set(old)), "only_in_parent_build": sorted(set(old) - set(new)),
               "changed": sorted(k for k in set(new) & set(old) if new[k] != old[k])}
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        Path(args.out).write_text(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
