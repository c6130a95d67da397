// Register / spill report of the ingest kernels without compiling the whole engine (VGPR spills in these kernels are
// not harmless on this toolchain: DESIGN.md section 4, "Skewed keys"). Usage:
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -c tools/regprobe.hip -o /tmp/rp.o \
//         -Rpass-analysis=kernel-resource-usage 2>&1 | grep -E "Function Name|VGPRs|Spill"
// or tools/regprobe.sh. The instantiations are the engine's own: the lists of flink_amd/csrc/ingest_launch.inc, which its
// launch tables expand too. -DREGPROBE_EXTRA='(const void*)&combine3_kernel<...>,' adds candidates, -DREGPROBE_ONLY_EXTRA
// leaves the lists out.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "../include/flink_amd.h"
#include "../flink_amd/csrc/java_math.h"

#define LONG_MIN_J ((int64_t)0x8000000000000000LL)
#define LONG_MAX_J ((int64_t)0x7fffffffffffffffLL)

namespace {
#include "../flink_amd/csrc/ingest.inc"
#include "../flink_amd/csrc/ingest_launch.inc"
}  // namespace

#define REGPROBE_P3(NV, IT, VW, KG, PRE, W16, NW, ROLL) (const void*)&partition3_kernel<NV, IT, 1024, VW, KG, PRE, W16, NW, ROLL>,
#define REGPROBE_C3(IT, NV, LY, PRE, MP, NW, LEAN) (const void*)&combine3_kernel<IT, 2, NV, 1024, LY, PRE, MP, NW, LEAN>,

const void* regprobe_kernels[] = {
#ifdef REGPROBE_EXTRA
    REGPROBE_EXTRA
#endif
#ifndef REGPROBE_ONLY_EXTRA
    FWA_P3_INSTANCES(REGPROBE_P3)
    FWA_C3_INSTANCES(REGPROBE_C3)
#endif
};
