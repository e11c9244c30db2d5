#!/bin/bash
# Print one line per kernel matching $1 (regex on the demangled name): VGPRs, AGPRs, scratch bytes per lane, occupancy, static
# LDS bytes per workgroup; with --spills also the SGPR and VGPR spill counts.  mlp_grad also lists the loss-carrying instances of
# t1d_mlp_loss (mlp_grad_kernel<T, LossArgs<T, kind>>) and the listed ones (.., TileArgs>), mlp_loss their sum kernel.  Extra
# hipcc flags after the pattern; the library's own (--offload-arch=gfx950 -O3 ...) come from simglucose_amd/_lib.py.  The figures
# are read from the device assembly that tools/kernel_asm.py compiles once per content and keeps under build/.
exec python3 "$(dirname "$0")/kernel_asm.py" "$@"
