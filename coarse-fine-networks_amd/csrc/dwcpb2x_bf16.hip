// dwcpb2x.hip compiled for bf16 tensors (cp_io.h): launcher dw_cpb2x_launch_bf16 and the C entry point
// hipcc-flags: -fno-slp-vectorize
#define DW_BF16 1
#include "dwcpb2x.hip"
