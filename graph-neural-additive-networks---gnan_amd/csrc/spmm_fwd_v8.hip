// The wide forward for operand rows read 8 floats per lane (bf16 rows): see csrc/spmm_fwd_body.hpp.
#include "spmm_fwd_body.hpp"

template int gnan::launch_lpr<8>(const gnan_spmm_args*, int, bool, bool, hipStream_t);
