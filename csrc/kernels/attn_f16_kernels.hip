// The fp16 instantiations of the attention kernels (attn_kernels.hip, attn_stream_kernels.hip:
// every kernel there takes a `bool F16`) and their launchers, launch_attn_*_f16.
//
// A translation unit of its own so that it has compile flags of its own (csrc/build.py
// SOURCE_FLAGS): this code is built without packed fp32 arithmetic, and the bf16 kernels keep the
// flags, and so the instructions, they were tuned and tested with.
#define DPT_ATTN_F16_UNIT 1
#include "attn_kernels.hip"
#include "attn_stream_kernels.hip"
