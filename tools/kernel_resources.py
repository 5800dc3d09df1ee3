#!/usr/bin/env python
"""Tabulate the compiler's kernel-resource-usage remarks (hipcc -Rpass-analysis=kernel-resource-usage, as the Makefile rule
of gauss_nested_kernel.hip asks for): one line per kernel with VGPRs, AGPRs, scratch, occupancy and LDS.  Needs no GPU.

    python tools/kernel_resources.py build.log        (the stderr of the compile)
"""
import re
import shutil
import subprocess
import sys

FIELDS = (("vgpr", r"VGPRs"), ("agpr", r"AGPRs"), ("scratch", r"ScratchSize \[bytes/lane\]"),
          ("occupancy", r"Occupancy \[waves/SIMD\]"), ("lds", r"LDS Size \[bytes/block\]"))


def main(path):
    text = open(path).read()
    seen = set()
    for block in re.split(r"remark: Function Name: ", text)[1:]:
        mangled = block.split("\n")[0].split(" [")[0].strip()
        if mangled in seen:
            continue
        seen.add(mangled)
        tool = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
        name = subprocess.run([tool, mangled], capture_output=True, text=True).stdout.strip() if tool else mangled
        name = re.sub(r"^void sqfa::|\(.*$", "", name)
        values = [re.search(pattern + r": (\d+)", block).group(1) for _, pattern in FIELDS]
        print(f"{name:70s} " + " ".join(f"{key} {value:>5}" for (key, _), value in zip(FIELDS, values)))


if __name__ == "__main__":
    main(sys.argv[1])
