#!/bin/bash
# Per-kernel registers / scratch / LDS of one .hip file of the engine, from the compiler's resource-usage remarks.
#   tools/kernel_resources.sh lunar_lander.hip
#   tools/kernel_resources.sh cartpole.hip -mllvm -amdgpu-kernarg-preload-count=14     (further compiler flags, e.g. the Makefile's per-object ones)
cd "$(dirname "$0")/../modurl_gym_amd/csrc" || exit 1
F="$1"; shift
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math "$@" -c "$F" -o /tmp/kres_$$.o \
    -Rpass-analysis=kernel-resource-usage 2>&1 |
  python3 -c '
import re, sys, subprocess
cur = None
for line in sys.stdin:
    m = re.search(r"remark:\s+(Function Name|TotalSGPRs|VGPRs|AGPRs|SGPRs Spill|VGPRs Spill|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)", line)
    if not m: continue
    k, v = m.groups()
    if k == "Function Name":
        cur = subprocess.run(["c++filt", v], capture_output=True, text=True).stdout.strip().split("(")[0]
        print()
        print(f"{cur:56s}", end="")
    else:
        name = "SGPRs" if k == "TotalSGPRs" else k.split()[0] + ("spill" if k.endswith("Spill") else "")
        print(f" {name}={v}", end="")
print()
'
rm -f /tmp/kres_$$.o
