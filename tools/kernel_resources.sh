#!/bin/bash
# register / scratch / LDS usage of every kernel of one translation unit (default physics_ll.hip; physics_ll.hip:regs = its register build),
# as the compiler reports it, compiled with the flags the library is built with (python -m vid2player3d_amd.build --print-flags)
F=${1:-physics_ll.hip}; cd "$(dirname "$0")/.."; FLAGS=$(python -m vid2player3d_amd.build --print-flags $F); cd vid2player3d_amd/csrc
/opt/rocm/bin/hipcc $FLAGS ${V2P_EXTRA_FLAGS:-} -Rpass-analysis=kernel-resource-usage -c ${F%%:*} -o /tmp/kr_$$.o 2>&1 |
  grep -E "Function Name|VGPRs:|AGPRs|Spill|ScratchSize|Occupancy|LDS Size|SGPRs:" | sed 's/.*remark: [^:]*:[0-9]*:[0-9]*: //' | paste - - - - - - - - - | sed 's/\[-Rpass-analysis=kernel-resource-usage\]//g' | tr -s ' '
rm -f /tmp/kr_$$.o
