// tmalign.hip — structural alignment search on the device (include/fdipt.h, "TM-align search"): for P pairs of
// CA traces, three initial alignments (gapless threading, secondary structure, secondary structure plus distance), each iterated by a
// dynamic programme under the transform of the seed search of section 7.8 (tmsearch.hpp), the d8 filter and the final scores per
// chain length, all in float64.  Modelled on Zhang & Skolnick's TM-align; the contract is this project's own, no parity is claimed.
//
// One launch, a block of 256 threads per pair, phases separated by barriers, everything in LDS (no workspace):
//   compact   x and y separately (ballot + popcount per wave, the waves' counts through LDS), with the original row of every kept row
//   Sec       a thread per row, classes as bytes
//   I1        a thread per offset of the threading, serial row walks; the selection of Fast is recomputed from the previous transform
//             instead of stored, so Fast needs no mask; one ordered argmax over the threads' candidates
//   DP        an anti-diagonal wavefront: thread t owns rows t + 1 and t + 257 and keeps its own row's last value, path bit and the
//             diagonal neighbour in registers; only the newest value and path bit of every row go through LDS (two buffers, one
//             barrier per diagonal).  Two bits of direction per cell, 16 cells of one row per word, so no two threads share a word;
//             the traceback is one thread's walk over the words
//   Search    tmsearch.hpp over the gathered pairs; its masks share their LDS with the directions (never live at the same time)
// inits = FDIPT_TMA_INITS_ALL launches tm_align5_kernel, the same block with the body's INITS5 switch on: behind I1 - I3 the candidates of
// I4 one after another on the whole block (a fragment superposition by one thread, DP, gather, Fast by one thread), then I5 as I1.
// Contraction into fused multiply-adds is off in this unit: the sums are compared with a NumPy evaluation in the same order.
#include "common.hpp"

#pragma clang fp contract(off)

#include "horn.hpp"
#include "tmsearch.hpp"
#include "tmalign_body.hpp"

template <bool INITS5>
__device__ __forceinline__ void tm_align_block(const FdiptTmAlignArgs a) {
  extern __shared__ double tma_sh[];
  __shared__ int cnt_sh[FD_THREADS / FD_WAVE], next_sh, passes_sh, count_sh;
  const int Na = a.N_a, Nb = a.N_b;
  const long p = blockIdx.x;
  const TmaOut o{a.tm, a.tm_a, a.tm_b, a.rotation, a.translation, a.rmsd, a.d0_a, a.d0_b, a.init_tm, a.alignment, a.n_aligned, a.init_dp, a.best_init, a.status, Nb};
  tma_clear<true, INITS5>(o, p, Nb);

  const int ia = a.pairs[2 * p], ib = a.pairs[2 * p + 1];
  const int Sb = a.prot_b ? a.S_b : a.S;
  if (ia < 0 || ia >= a.S || ib < 0 || ib >= Sb) {  // the device data decide what is addressed
    tma_leave<true>(o, p, FDIPT_TMA_SKIPPED, 0, 0.0, 0.0, -1);
    return;
  }
  const TmaSource A{a.prot + ((long)ia * Na * a.atoms + a.ca) * 3, a.mask + (long)ia * Na, (long)a.atoms * 3, Na};
  const TmaSource B{a.prot_b ? a.prot_b + ((long)ib * Nb * a.atoms_b + a.ca) * 3 : a.prot + ((long)ib * Nb * a.atoms + a.ca) * 3,
                    (a.prot_b ? a.mask_b : a.mask) + (long)ib * Nb, (long)(a.prot_b ? a.atoms_b : a.atoms) * 3, Nb};
  tma_pair<true, true, INITS5>(A, B, Na, Nb, o, p, tma_sh, cnt_sh, &next_sh, &passes_sh, &count_sh, TmaNoEarly());
}

__global__ __launch_bounds__(FD_THREADS) void tm_align_kernel(FdiptTmAlignArgs a) { tm_align_block<false>(a); }
__global__ __launch_bounds__(FD_THREADS) void tm_align5_kernel(FdiptTmAlignArgs a) { tm_align_block<true>(a); }

extern "C" size_t fdipt_sample_tm_align_workspace(int S, int N_a, int N_b, int P) {
  (void)S, (void)N_a, (void)N_b, (void)P;  // the search lives in LDS and registers; the entry keeps the arguments for a later layout
  return 0;
}

extern "C" int fdipt_sample_tm_align(const FdiptTmAlignArgs* a, fdipt_stream_t stream) {
  if (!a || a->S < 1 || a->N_a < 1 || a->N_b < 1 || a->P < 1 || (a->atoms != 37 && a->atoms != 5) || a->ca < 0 || a->ca >= 5) return FDIPT_EINVAL;
  if (!a->prot || !a->mask || !a->pairs || !a->tm || !a->tm_a || !a->tm_b || !a->rotation || !a->translation || !a->alignment || !a->n_aligned ||
      !a->rmsd || !a->d0_a || !a->d0_b || !a->init_tm || !a->init_dp || !a->best_init || !a->status)
    return FDIPT_EINVAL;
  if (a->prot_b && (!a->mask_b || a->S_b < 1 || (a->atoms_b != 37 && a->atoms_b != 5))) return FDIPT_EINVAL;
  if (!a->prot_b && a->N_b != a->N_a) return FDIPT_EINVAL;
  if (a->inits != FDIPT_TMA_INITS_DEFAULT && a->inits != FDIPT_TMA_INITS_ALL) return FDIPT_EINVAL;
  if (a->N_a > TMA_MAX_ROWS || a->N_b > TMA_MAX_ROWS) return FDIPT_ESIZE;
  if (a->workspace_bytes < fdipt_sample_tm_align_workspace(a->S, a->N_a, a->N_b, a->P)) return FDIPT_ESIZE;
  const bool five = a->inits == FDIPT_TMA_INITS_ALL;
  const size_t lds = tma_layout(a->N_a, a->N_b, five).total;
  static FdPerDevice attr_dev;
  const int dev_ = fd_device();
  if (!attr_dev.get(dev_)) {  // 512 x 512: 131 KB (132 KB with the five starts), more than the default 64 KB of dynamic LDS
    if (hipFuncSetAttribute((const void*)tm_align_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)tma_layout(TMA_MAX_ROWS, TMA_MAX_ROWS).total) !=
            hipSuccess ||
        hipFuncSetAttribute((const void*)tm_align5_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)tma_layout(TMA_MAX_ROWS, TMA_MAX_ROWS, true).total) != hipSuccess)
      return FDIPT_ELAUNCH;
    attr_dev.set(dev_, 1);
  }
  if (five) hipLaunchKernelGGL(tm_align5_kernel, dim3((unsigned)a->P), dim3(FD_THREADS), lds, (hipStream_t)stream, *a);
  else hipLaunchKernelGGL(tm_align_kernel, dim3((unsigned)a->P), dim3(FD_THREADS), lds, (hipStream_t)stream, *a);
  FD_CHECK_LAUNCH();
  return FDIPT_OK;
}
