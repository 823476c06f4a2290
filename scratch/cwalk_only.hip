// cwalk_only.hip -- the candidate-pool walkers alone, for reading the compiler's output without building the whole library:
// one explicit instantiation per compile (58 in all: 43 k_cwalk, 13 k_cwalk2, 2 k_cwalkg -- the set launch_cw_path dispatches to).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -Iinclude -Igretel_amd/csrc --cuda-device-only -S \
//         -DCW_ONLY='k_cwalk2<64, 4>' -o out.s scratch/cwalk_only.hip
// scratch/cwalk_isa.py runs all of them for a source tree and compares two such runs.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <utility>
#include "gretel_hip.h"
#include "gh_detlog.h"
#include "kernels.hpp"
#include "segwalk.hpp"
#include "cwalk.hpp"

template __global__ void CW_ONLY(cw_params);
