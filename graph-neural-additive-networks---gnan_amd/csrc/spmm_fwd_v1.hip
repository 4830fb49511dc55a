// The wide forward for operand rows read 1 float per lane: see csrc/spmm_fwd_body.hpp.
#include "spmm_fwd_body.hpp"

template int gnan::launch_lpr<1>(const gnan_spmm_args*, int, bool, bool, hipStream_t);
