#!/bin/bash
# Register, scratch, spill and occupancy figures of every merge_small_kernel instantiation, as the
# compiler reports them (-Rpass-analysis=kernel-resource-usage); needs no GPU.  Extra arguments
# go to the compiler (e.g. -DHM_WAVES_PER_EU=4).  The instantiation is <OPL, LISTS, size class>.
#   tools/kernel_resources.sh [flags...] > profiles/<round>/<name>.txt
# HM_KERNEL_SRC=<file of csrc/> (e.g. past_kernels.hip): every kernel of that file instead, with its LDS.
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
ARCH=${HM_OFFLOAD_ARCH:-gfx950}
$HIPCC --offload-arch=$ARCH -O3 -std=c++17 -fPIC -mllvm -amdgpu-atomic-optimizer-strategy=DPP \
    --cuda-device-only -c -o /dev/null -Rpass-analysis=kernel-resource-usage "$@" \
    "$R/hypermerge_amd/csrc/${HM_KERNEL_SRC:-merge_kernels.hip}" 2>&1 | HM_KERNEL_SRC="$HM_KERNEL_SRC" python3 -c '
import os, re, subprocess, sys
rows, cur = [], None
for line in sys.stdin:
    m = re.search(r"remark: .*Function Name: (\S+)", line)
    if m:
        cur = {"name": m.group(1)}
        rows.append(cur)
        continue
    m = re.search(r"remark: .*?\s{2,}([A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+)\s*\[-Rpass", line)
    if m and cur is not None:
        cur[m.group(1).strip()] = m.group(2)
if os.environ.get("HM_KERNEL_SRC"):
    print("%-44s %6s %6s %8s %9s %9s %5s %7s" % ("kernel", "VGPRs", "SGPRs", "scratch", "SGPRspill", "VGPRspill", "occ", "LDS"))
    for r in rows:
        name = subprocess.run(["c++filt", "-p", r["name"]], capture_output=True, text=True).stdout.strip() or r["name"]
        print("%-44s %6s %6s %8s %9s %9s %5s %7s" % (name, r.get("VGPRs"), r.get("TotalSGPRs"), r.get("ScratchSize"),
                                                     r.get("SGPRs Spill"), r.get("VGPRs Spill"), r.get("Occupancy"), r.get("LDS Size")))
    sys.exit(0)
print("%-24s %6s %6s %8s %9s %9s %5s" % ("merge_small_kernel<>", "VGPRs", "SGPRs", "scratch", "SGPRspill", "VGPRspill", "occ"))
for r in rows:
    m = re.match(r"_ZN2hm18merge_small_kernelILi(\d)ELb(\d)ELi(\d)EEEv", r["name"])
    if not m:
        continue
    inst = "<%s, %s, %s>" % (m.group(1), "true" if m.group(2) == "1" else "false", m.group(3))
    print("%-24s %6s %6s %8s %9s %9s %5s" % (inst, r.get("VGPRs"), r.get("TotalSGPRs"), r.get("ScratchSize"),
                                             r.get("SGPRs Spill"), r.get("VGPRs Spill"), r.get("Occupancy")))
'
