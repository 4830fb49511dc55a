// The wide forward for operand rows read 4 floats per lane: see csrc/spmm_fwd_body.hpp.
#include "spmm_fwd_body.hpp"

template int gnan::launch_lpr<4>(const gnan_spmm_args*, int, bool, bool, hipStream_t);
