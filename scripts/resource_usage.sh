#!/bin/bash
# Code-object resource notes of every kernel (VGPR / AGPR / SGPR spills / scratch / occupancy / LDS), from the
# compiler's kernel-resource-usage remarks on the same flags as the Makefile.  Runs on the CPU (cross-compile).
# usage: bash scripts/resource_usage.sh [file.hip ...] > profiles/<tag>_resources.txt   (no files: every kernel source)
set -euo pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
cd "$ROOT/rapid-locomotion-rl_amd/csrc"
ALL="lrl_env_dispatch.hip lrl_env_flat.hip lrl_env_mesh.hip lrl_env_mesh_tgs.hip lrl_aux.hip lrl_gae.hip lrl_gemm.hip lrl_ppo.hip lrl_curriculum_dev.hip lrl_render.hip lrl_depth.hip lrl_vision.hip"
for f in ${@:-$ALL}; do
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=fast-honor-pragmas \
    -Xclang -target-feature -Xclang -packed-fp32-ops --cuda-device-only \
    -Rpass-analysis=kernel-resource-usage -c "$f" -o /tmp/lrl_res_$$.o 2>&1 |
    sed -n 's/.*remark: *//p' | sed 's/ \[-Rpass-analysis=kernel-resource-usage\]//' |
    awk -v F="$f" '/^Function Name:/ {printf "\n%s %s", F, $3; next}
                   /^(VGPRs|AGPRs|ScratchSize|Occupancy|SGPRs Spill|VGPRs Spill|LDS Size)/ {printf " | %s", $0}'
done
echo
rm -f /tmp/lrl_res_$$.o
