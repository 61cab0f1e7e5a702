// gdt.hip — GDT-TS / GDT-HA of samples on the device (include/fdipt.h, "GDT-TS / GDT-HA"): for P pairs (model,
// reference) in row correspondence the number of rows within 0.5, 1, 2, 4 and 8 Angstrom under the identity (NONE: the frame of the
// fixed context, openfold's gdt on the raw coordinates), under one least-squares superposition of all rows (GLOBAL: superimpose, then
// gdt) or, per cutoff, under the best transform a seed search visits (SEARCH), all in float64.
//
// One launch, a block per pair, no workspace traffic.  The compaction and the LDS layout are tmscore.hip's: six coordinate arrays, two
// bit masks per thread, a reduction area - here five (count, item, pass) triples per thread - and behind it the row of every compacted
// position (res_within is indexed by row).
//   SEARCH: a work item is (refinement cutoff k, seed of tmsearch.hpp's ladder, every start), numbered k * n_seeds + seed.  The loop is
//       flat like tm_search's: an iteration is one pass of whatever item the lane holds - superpose the set (tm_superpose), walk the rows
//       once for the five counts and the next set (d^2 < cut^2, cut = c_k, widened as tm_search widens it) - and a lane whose item ends
//       takes the next number from a counter in LDS.  Every pass offers its five counts to the lane's five running maxima.  Five best
//       transforms per thread would be 60 doubles of registers or 122 KB of LDS, so a thread keeps (count, item, pass) only; after one
//       ordered reduction per cutoff (largest count, lowest item, earliest pass) lane j of the block replays the winner of cutoff j to
//       its pass and so obtains its transform.  Which lane serves which item depends on timing; no output does.
//   GLOBAL: thread 0 superposes all rows.  NONE: the identity.
//   Then the whole block walks the rows in parallel under the five transforms: res_within, and in NONE and GLOBAL the counts
//   (ballot + popcount, integer adds in LDS).
// Contraction into fused multiply-adds is off in this unit: the distances are compared with a NumPy evaluation in the same order.
#include "gdt_body.hpp"

__global__ __launch_bounds__(FD_THREADS) void gdt_kernel(FdiptGdtArgs a) { gdt_body<false>(a, FdiptRowMap{}); }

extern "C" size_t fdipt_sample_gdt_workspace(int S, int N, int P) {
  (void)S, (void)N, (void)P;  // the search lives in LDS and registers; the entry keeps the argument for a later layout
  return 0;
}

extern "C" int fdipt_sample_gdt(const FdiptGdtArgs* a, fdipt_stream_t stream) {
  if (!a || a->S < 1 || a->N < 1 || a->P < 1 || (a->atoms != 37 && a->atoms != 5) || a->ca < 0 || a->ca >= 5) return FDIPT_EINVAL;
  if (a->mode != FDIPT_GDT_NONE && a->mode != FDIPT_GDT_GLOBAL && a->mode != FDIPT_GDT_SEARCH) return FDIPT_EINVAL;
  if (!a->prot || !a->mask || !a->pairs || !a->gdt_ts || !a->gdt_ha || !a->counts || !a->n_scored || !a->rotation || !a->translation || !a->best_item ||
      !a->best_pass || !a->passes || !a->res_within || !a->status)
    return FDIPT_EINVAL;
  if (a->prot_b && (!a->mask_b || a->S_b < 1 || (a->atoms_b != 37 && a->atoms_b != 5))) return FDIPT_EINVAL;
  if (a->N > FDIPT_TM_MAX_ROWS) return FDIPT_ESIZE;
  if (a->workspace_bytes < fdipt_sample_gdt_workspace(a->S, a->N, a->P)) return FDIPT_ESIZE;
  const size_t lds = gdt_lds_bytes(a->N);
  static FdPerDevice attr_dev;
  const int dev_ = fd_device();
  if (!attr_dev.get(dev_)) {  // N = 1024: 131 KB, more than the default 64 KB of dynamic LDS
    if (hipFuncSetAttribute((const void*)gdt_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)gdt_lds_bytes(FDIPT_TM_MAX_ROWS)) != hipSuccess)
      return FDIPT_ELAUNCH;
    attr_dev.set(dev_, 1);
  }
  hipLaunchKernelGGL(gdt_kernel, dim3((unsigned)a->P), dim3(FD_THREADS), lds, (hipStream_t)stream, *a);
  FD_CHECK_LAUNCH();
  return FDIPT_OK;
}
