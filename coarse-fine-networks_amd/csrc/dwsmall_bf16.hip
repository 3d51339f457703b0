// dwsmall.hip compiled for bf16 tensors (cp_io.h): launcher dw_small_launch_bf16
#define DW_BF16 1
#include "dwsmall.hip"
