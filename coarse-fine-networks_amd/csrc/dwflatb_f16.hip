// dwflatb.hip compiled for fp16 tensors (cp_io.h): launcher dw_flatb_launch_f16
// hipcc-flags: -fno-slp-vectorize
#define DW_BF16 1
#define CFN_F16 1
#include "dwflatb.hip"
