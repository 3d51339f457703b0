#!/bin/bash
# Knock-out table of the one-pass split-bf16 pointwise backward (csrc/pwfuseds.hip): parts of the kernel switched off through CFN_PWFS_DBG
# (1 weight gradient, 2 data gradient, 4 act' / statistics epilogue, 8 gx stores) -- results are wrong, times tell where a stage goes.
# The product library does not read CFN_PWFS_DBG: the table runs on a variant built with -DCFN_PWFS_KNOCKOUTS and selected through CFN_HIP_LIB.
# Build the variant where the library was built (it needs the object files):  tools/pwfs_knockouts.sh build ; the table itself needs a GPU.
R=$(cd "$(dirname "$0")/.." && pwd)
KO=$R/coarse-fine-networks_amd/cfn_hip/variants/libcfn_hip_knockouts.so
if [ "$1" = build ]; then exec bash $R/tools/variant_lib.sh knockouts pwfuseds.hip "-fno-slp-vectorize -DCFN_PWFS_KNOCKOUTS"; fi
[ -f $KO ] || { echo "$KO is missing: run  tools/pwfs_knockouts.sh build  first" >&2; exit 1; }
for d in 0 1 2 3 4 8 7 15; do
  echo "## CFN_PWFS_DBG=$d"
  CFN_HIP_LIB=$KO CFN_PWF_SPLIT=2 CFN_PWFS_DBG=$d python $R/tools/pwfs_bench.py 2>&1 | grep "fused" | sed 's/separate [0-9.]* ms *//'
done
