// seqalign_modes.hip — sequence alignment with a mode: global, semi-global (chosen end gaps free) and local, for P pairs of sequences:
// fdipt_seq_align_modes (include/fdipt.h, "sequence alignment: modes").
//
// The kernels are seqalign_body.hpp's, in its policies SQ_ENDS (semi-global; without a flag that is the global mode, so one
// instantiation serves both) and SQ_LOCAL: the end cell is a choice, and the result carries the span of the charged path.
#include "seqalign_body.hpp"

template <int MODE, bool TRACE>
__global__ __launch_bounds__(FD_THREADS) void seq_align_modes_kernel(FdiptSeqAlignModeArgs a, int W, int wpb) {
  seq_align_body<MODE == FDIPT_SEQ_MODE_LOCAL ? SQ_LOCAL : SQ_ENDS, TRACE>(a, W, wpb);
}

extern "C" size_t fdipt_seq_align_modes_workspace_bytes(int P, int max_len_a, int max_len_b, int traceback, size_t max_workspace_bytes) {
  return sq_workspace_bytes(P, max_len_a, max_len_b, traceback, max_workspace_bytes, sq_extra(SQ_ENDS));
}

extern "C" int fdipt_seq_align_modes(const FdiptSeqAlignModeArgs* a, fdipt_stream_t stream) {
  // (this entry's own checks come first; every refusal up to the size check is FDIPT_EINVAL, so their order decides nothing)
  if (!a || !a->begin_a || !a->end_a || !a->begin_b || !a->end_b) return FDIPT_EINVAL;
  if (a->mode != FDIPT_SEQ_MODE_GLOBAL && a->mode != FDIPT_SEQ_MODE_SEMIGLOBAL && a->mode != FDIPT_SEQ_MODE_LOCAL) return FDIPT_EINVAL;
  if (a->free_ends < 0 || a->free_ends > 15 || (a->free_ends && a->mode != FDIPT_SEQ_MODE_SEMIGLOBAL)) return FDIPT_EINVAL;
  int rc = sq_check_args(a), W, wpb;
  size_t lds;
  if (rc != FDIPT_OK || (rc = sq_plan_launch(a, sq_extra(SQ_ENDS), W, wpb, lds)) != FDIPT_OK) return rc;
  static FdPerDevice attr_dev[2][2];  // per kernel
  static void (*const kernels[2][2])(FdiptSeqAlignModeArgs, int, int) = {
      {seq_align_modes_kernel<FDIPT_SEQ_MODE_SEMIGLOBAL, false>, seq_align_modes_kernel<FDIPT_SEQ_MODE_SEMIGLOBAL, true>},
      {seq_align_modes_kernel<FDIPT_SEQ_MODE_LOCAL, false>, seq_align_modes_kernel<FDIPT_SEQ_MODE_LOCAL, true>}};
  const int local = a->mode == FDIPT_SEQ_MODE_LOCAL, trace = a->traceback != 0;
  return sq_launch(kernels[local][trace], attr_dev[local][trace], a, W, wpb, lds, (hipStream_t)stream);
}
