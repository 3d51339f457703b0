// dwsmall.hip compiled for fp16 tensors (cp_io.h): launcher dw_small_launch_f16
#define DW_BF16 1
#define CFN_F16 1
#include "dwsmall.hip"
