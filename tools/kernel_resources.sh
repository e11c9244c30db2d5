#!/bin/bash
# Compile the library with -Rpass-analysis=kernel-resource-usage and print one line per kernel matching $1 (regex on the
# demangled name): VGPRs, AGPRs, scratch bytes per lane, occupancy, static LDS bytes per workgroup.  mlp_grad also lists the loss-carrying instances of
# t1d_mlp_loss (mlp_grad_kernel<T, LossArgs<T, kind>>) and the listed ones (.., TileArgs>), mlp_loss their sum kernel.  Extra
# hipcc flags after the pattern; the library's own (--offload-arch=gfx950 -O3 ...) come from simglucose_amd/_lib.py.
pat="${1:-.}"; shift
root="$(cd "$(dirname "$0")/.." && pwd)"
flags="$(cd "$root" && python3 -c 'from simglucose_amd._lib import HIPCC_FLAGS; print(*HIPCC_FLAGS)')" || exit 1
/opt/rocm/bin/hipcc $flags -shared -fPIC -Rpass-analysis=kernel-resource-usage "$@" \
    -o /tmp/libt1d_res.so "$root/simglucose_amd/csrc/t1d_abi.hip" 2>&1 |
  awk '/Function Name:/ {name=$0; sub(/.*Function Name: /,"",name); sub(/ \[-R.*/,"",name)}
       / VGPRs:/ {v=$(NF-1)} / AGPRs:/ {a=$(NF-1)} /ScratchSize/ {s=$(NF-1)} /Occupancy/ {o=$(NF-1)}
       /LDS Size/ {print name, "vgpr", v, "agpr", a, "scratch", s, "occ", o, "lds", $(NF-1)}
       /error/ {print}' | while read n rest; do echo "$(echo $n | c++filt) $rest"; done | grep -E "$pat"
