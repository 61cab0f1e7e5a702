// seqalign.hip — global sequence alignment with affine gaps (Gotoh, three states) for P pairs of sequences: fdipt_seq_align
// (include/fdipt.h, "sequence alignment").
//
// The kernels are seqalign_body.hpp's, in its policy SQ_PLAIN: the end cell is (la, lb) and no state carries an origin.
#include "seqalign_body.hpp"

template <bool TRACE>
__global__ __launch_bounds__(FD_THREADS) void seq_align_kernel(FdiptSeqAlignArgs a, int W, int wpb) {
  seq_align_body<SQ_PLAIN, TRACE>(a, W, wpb);
}

extern "C" size_t fdipt_seq_align_workspace_bytes(int P, int max_len_a, int max_len_b, int traceback, size_t max_workspace_bytes) {
  return sq_workspace_bytes(P, max_len_a, max_len_b, traceback, max_workspace_bytes, sq_extra(SQ_PLAIN));
}

extern "C" int fdipt_seq_align(const FdiptSeqAlignArgs* a, fdipt_stream_t stream) {
  int rc = sq_check_args(a), W, wpb;
  size_t lds;
  if (rc != FDIPT_OK || (rc = sq_plan_launch(a, sq_extra(SQ_PLAIN), W, wpb, lds)) != FDIPT_OK) return rc;
  static FdPerDevice attr_dev[2];  // per kernel
  return sq_launch(a->traceback ? seq_align_kernel<true> : seq_align_kernel<false>, attr_dev[a->traceback != 0], a, W, wpb, lds, (hipStream_t)stream);
}
