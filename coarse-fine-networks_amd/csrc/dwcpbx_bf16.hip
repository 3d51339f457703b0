// dwcpbx.hip compiled for bf16 tensors (cp_io.h): launcher dw_cpbx_launch_bf16
// hipcc-flags: -fno-slp-vectorize
#define DW_BF16 1
#include "dwcpbx.hip"
