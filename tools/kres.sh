#!/bin/bash
# compact table: template flags (CONTACT MULTI TGS DIAG BALL JOBS LIMITS) / VGPRs / scratch bytes per lane / occupancy of every physics_ll_kernel
# instantiation as the compiler reports it (CPU only).  Usage: tools/kres.sh [--regs] [extra -D flags]   (--regs: the flags of the library's
# second, register build; the flags are build.py's own: python -m vid2player3d_amd.build --print-flags)
#        tools/kres.sh --source mvae_player.hip [extra flags]: the same for every kernel of another source of the library (name, VGPRs, AGPRs,
# scratch bytes per lane, occupancy, LDS bytes per workgroup)
if [ "$1" = "--source" ]; then
  S=$2; shift 2
  cd "$(dirname "$0")/.."; FLAGS=$(python -m vid2player3d_amd.build --print-flags $S); cd vid2player3d_amd/csrc
  /opt/rocm/bin/hipcc $FLAGS "$@" -Rpass-analysis=kernel-resource-usage -c $S -o /tmp/kres_$$.o 2>&1 |
    grep -E "Function Name|VGPRs:|AGPRs:|ScratchSize|Occupancy|LDS Size" | sed 's/.*remark: *//; s/ *\[-Rpass-analysis=kernel-resource-usage\]//' | paste - - - - - - |
    sed "s/Function Name: //; s/ScratchSize \[bytes\/lane\]/scratch/; s/Occupancy \[waves\/SIMD\]/occ/; s/LDS Size \[bytes\/block\]/LDS/" | tr -s " \t" " "
  rm -f /tmp/kres_$$.o
  exit 0
fi
S=physics_ll.hip; if [ "$1" = "--regs" ]; then shift; S=physics_ll.hip:regs; fi
cd "$(dirname "$0")/.."; FLAGS=$(python -m vid2player3d_amd.build --print-flags $S); cd vid2player3d_amd/csrc
/opt/rocm/bin/hipcc $FLAGS "$@" -Rpass-analysis=kernel-resource-usage -c physics_ll.hip -o /tmp/kres_$$.o 2>&1 |
  grep -E "Function Name|VGPRs:|ScratchSize|Occupancy" | sed 's/.*remark: [^:]*:[0-9]*:[0-9]*: //; s/\[-Rpass-analysis=kernel-resource-usage\]//' | paste - - - - |
  grep physics_ll_kernel | sed 's/Function Name: _ZN3v2p[0-9]*ll_[a-z]*17physics_ll_kernelI//; s/EEvNS_8PhysArgsE//; s/Lb//g; s/E/ /g' | sed "s/physics_ll.hip:[0-9]*:[0-9]*: remark: //g; s/ScratchSize \[bytes\/lane\]/scratch/; s/Occupancy \[waves\/SIMD\]/occ/" | tr -s " \t" " "
rm -f /tmp/kres_$$.o
